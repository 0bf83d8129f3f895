"""CPU: the pins of the long-double yardstick tests/_sat_ref.py, the record of
where the fp64 yardsticks break, and the preconditions of the steep designs
tests/test_gpu_saturated.py fits -- no GPU.

* Against mpmath at 50 digits on the grid of posed rows: every term of
  ``_sat_ref.row_terms_ld`` within 8 long-double eps relative.  The mpmath
  statements take mu and 1 - mu as 1 / (1 + exp(-+eta)), each of which is
  accurate at any working precision, and the logs through log1p.
* On |eta| <= 20 ``_sat_ref`` agrees with ``_gof_ref.row_terms`` and
  ``_glm_ref.loglik`` within the bounds tests/test_cpu_gof.py states.
* Today's holes of the fp64 form: ``_gof_ref.row_terms`` is 0 at the matched
  logistic rows from |eta| = 37 on and NaN once exp(-|eta|) is 0; the Poisson
  form is NaN at y = 0 over an underflowed mu and at an overflowed mu.
* The steep designs converge, are well conditioned and have the saturated rows
  the GPU tests are about; the emulator ends "ok" without an escalation.
"""

import functools

import numpy as np
import pytest

import _glm_ref as G
import _gof_ref as R
import _newton_ref as N
import _sat_ref as S

LD = S.LD
EPS_LD = float(np.finfo(LD).eps)


def _mp_terms(family, y, eta, om):
    """The six terms of one row with mpmath at 50 digits."""
    import mpmath as mp

    mp.mp.dps = 50
    y, eta, om = mp.mpf(float(y)), mp.mpf(float(eta)), mp.mpf(float(om))
    if family == "poisson":
        mu = mp.exp(eta)
        ll = y * eta - mu - mp.loggamma(y + 1)
        dev = 2 * (y * (mp.log(y) - eta) - (y - mu)) if y > 0 else 2 * mu
        return dict(loglik=om * ll, deviance=om * dev, pearson=om * (y - mu) ** 2 / mu, mu=mu,
                    w=om * mu, s=om * (y - mu))
    p, q = 1 / (1 + mp.exp(-eta)), 1 / (1 + mp.exp(eta))  # mu and 1 - mu
    logp, logq = -mp.log1p(mp.exp(-eta)), -mp.log1p(mp.exp(eta))
    ll = y * logp + (1 - y) * logq
    sat = (y * mp.log(y) if y > 0 else 0) + ((1 - y) * mp.log(1 - y) if y < 1 else 0)
    r = q if y == 1 else (-p if y == 0 else y - p)
    return dict(loglik=om * ll, deviance=2 * om * (sat - ll), pearson=om * r * r / (p * q), mu=p,
                w=om * p * q, s=om * r)


@pytest.mark.parametrize("family", ["logistic", "poisson"])
def test_long_double_terms_against_mpmath(family):
    import mpmath as mp

    y, eta, om = S.grid_rows(family)
    got = S.row_terms_ld(family, y, eta, om)
    lo, hi = mp.mpf(10) ** -4900, mp.mpf(10) ** 4900  # inside the long double normals
    worst = 0.0
    for i in range(len(y)):
        want = _mp_terms(family, y[i], eta[i], om[i])
        for k in S.KEYS:
            g, w = got[k][i], want[k]
            if abs(w) > hi:
                assert np.isinf(g) and (g > 0) == (w > 0), (family, k, y[i], eta[i], g)
            elif abs(w) < lo:
                assert g == 0, (family, k, y[i], eta[i], g)
            else:
                # the long double as an exact mpf: its 64-bit significand and exponent
                m, e = np.frexp(g)
                gm = mp.mpf(int(np.ldexp(m, 64))) * mp.mpf(2) ** (int(e) - 64)
                # relative to the value; the Poisson deviance y (log y - eta) - (y - mu)
                # cancels in any form where y is near mu, and is held to the size
                # of its two terms instead (the fp64 bound is 2^11 times that)
                size = abs(w)
                if family == "poisson" and k == "deviance" and y[i] > 0:
                    size = 2 * om[i] * (abs(want["loglik"] / om[i] + want["mu"]) + abs(y[i] - want["mu"]))
                rel = float(abs(gm - w) / size)
                worst = max(worst, rel)
                assert rel <= 8 * EPS_LD, (family, k, y[i], eta[i], rel / EPS_LD)
    print(f"{family}: worst relative error {worst / EPS_LD:.2f} long-double eps over {len(y)} rows")


def test_rounding_to_fp64_overflows_and_underflows():
    t = S.row_terms("logistic", [0.0, 1.0, 0.0, 1.0], [800.0, 800.0, -745.0, 1e5])
    assert t["pearson"].tolist() == [np.inf, 0.0, 5e-324, 0.0]
    t = S.row_terms("poisson", [0.0, 3.0, 3.0], [-800.0, -800.0, 800.0])
    assert t["pearson"].tolist() == [0.0, np.inf, np.inf] and t["s"][2] == -np.inf
    assert t["deviance"][2] == np.inf and t["loglik"][2] == -np.inf


@pytest.mark.parametrize("family", ["logistic", "poisson"])
def test_agrees_with_the_fp64_yardsticks_where_they_are_sound(family):
    """|eta| <= 20 (Poisson 5): partition sums within test_cpu_gof.py's REL =
    1e-12, rows within its Pearson bound 32 eps plus the conditioning of y -
    mu; the log-likelihood sum against ``_glm_ref.loglik``."""
    rng = np.random.default_rng(12)
    n = 4000
    eta = np.concatenate([rng.uniform(-20, 20, n - 4), [-20.0, 20.0, 0.0, 1e-9]])
    w = rng.uniform(0.2, 5.0, n)
    if family == "logistic":
        y = np.round(rng.random(n))
    else:
        eta = eta / 4.0
        y = rng.poisson(np.exp(eta)).astype(np.float64)
    t = S.row_terms(family, y, eta, w)
    d, c = R.row_terms(family, y, eta, w)
    eps = np.finfo(np.float64).eps
    assert abs(d.sum() - t["deviance"].sum()) <= 1e-12 * t["deviance"].sum()
    assert abs(c.sum() - t["pearson"].sum()) <= 1e-12 * t["pearson"].sum()
    mu = t["mu"]
    cond = 8 * eps * (y + mu) / np.maximum(np.abs(y - mu), np.finfo(np.float64).tiny)
    assert (np.abs(c - t["pearson"]) <= (32 * eps + cond) * t["pearson"] + 1e-300).all()
    ll = G.loglik(family, eta[:, None], y, np.ones(1), w)
    assert abs(ll - t["loglik"].sum()) <= 1e-12 * abs(t["loglik"].sum())
    # w and s against _glm_ref's (mu, omega w)
    mu_g, v_g = G._mu_w(family, eta[:, None], np.ones(1), w, None)
    # (_glm_ref forms 1 - mu and y - mu, each rounded at eps of 1, or of y + mu)
    assert (np.abs(v_g - t["w"]) <= 32 * eps * t["w"] + 2 * eps * w).all()
    assert (np.abs(w * (y - mu_g) - t["s"]) <= 4 * eps * w * np.maximum(1.0, y + mu)).all()


def test_the_holes_of_the_fp64_form():
    """Why tests/_sat_ref.py exists: at these rows ``_gof_ref.row_terms`` (the
    form the kernels had) is 0 or NaN where the value is neither."""
    y, eta, om = S.grid_rows("logistic")
    with np.errstate(all="ignore"):
        _, chi = R.row_terms("logistic", y, eta, om)
    ref = S.row_terms("logistic", y, eta, om)["pearson"]
    assert not np.isnan(ref).any()
    matched = ((y == 1) & (eta > 0)) | ((y == 0) & (eta < 0))
    # y (1 + ea) - 1 cancels to 0 (the mirror image, 0 (1 + ea) - ea, is exact)
    quiet = (y == 1) & (eta >= 37) & (eta <= 745)
    assert quiet.sum() == 10 and (chi[quiet] == 0).all() and (ref[quiet] > 0).all()
    assert ref[quiet].max() == pytest.approx(np.exp(-37.0), rel=1e-15)
    gone = matched & (np.abs(eta) > 745.2)  # ea = 0: 0 / 0
    assert gone.sum() == 2 * 4 and np.isnan(chi[gone]).all() and (ref[gone] == 0).all()
    # every other posed row is sound in both
    rest = ~(quiet | gone)
    assert not np.isnan(chi[rest]).any()

    y, eta, om = S.grid_rows("poisson")
    with np.errstate(all="ignore"):
        _, chi = R.row_terms("poisson", y, eta, om)
    ref = S.row_terms("poisson", y, eta, om)["pearson"]
    assert not np.isnan(ref).any()
    dead = (y == 0) & (eta < -745.2)       # mu = 0: 0 / 0 where the value is mu -> 0
    assert dead.sum() == 3 and np.isnan(chi[dead]).all() and (ref[dead] == 0).all()
    over = eta > 709.9                     # mu = inf: inf * inf / inf where the value is +inf
    assert over.sum() == 2 * len(S.POISSON_Y) and np.isnan(chi[over]).all()
    assert (ref[over] == np.inf).all()
    sq = (eta >= 500) & ~over              # (y - mu)^2 overflows where the value, ~mu, does not
    assert (chi[sq] == np.inf).all() and np.isfinite(ref[sq]).all()


# ---- the steep designs --------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _steep(name):
    p, sizes, seed = S.STEEP[name]
    off = S.offsets_of(sizes)
    X, y, _ = S.steep_design(int(off[-1]), p, seed)
    return X, y, off, G.fit_partitions("logistic", X, y, off, fit_intercept=True)


@pytest.mark.parametrize("name", list(S.STEEP))
def test_steep_designs_are_easy_fits_with_saturated_rows(name):
    X, y, off, ref = _steep(name)
    Z = G.design(X, True)
    best = (0, 0)
    for k, (a, b) in enumerate(zip(off[:-1], off[1:])):
        assert ref["iters"][k] < 50 and np.isfinite(ref["theta"][k]).all()
        assert np.isfinite(ref["sig_inv"][k]).all() and np.isfinite(ref["loglik"][k])
        cond = np.linalg.cond(ref["sig_inv"][k])
        ae = np.abs(Z[a:b] @ ref["theta"][k])
        gone, far = int((ae > 745.13).sum()), int(((ae > 40) & (ae < 700)).sum())
        print(f"{name} partition {k}: iters {ref['iters'][k]} halvings {ref['halvings'][k]} "
              f"cond {cond:.1f} rows past 745.13: {gone}, in (40, 700): {far}")
        assert cond < 1e3
        if gone >= 10 and far >= 100:
            best = (gone, far)
        # the fp64 form's Pearson sum is NaN exactly where a row is past 745.13
        with np.errstate(all="ignore"):
            chi = R.gof("logistic", Z[a:b], y[a:b], ref["theta"][k])[1]
        assert np.isnan(chi) == (gone > 0)
        t = S.row_terms("logistic", y[a:b], S.eta_ld(Z[a:b], ref["theta"][k]))
        assert np.isfinite(t["pearson"].sum()) and np.isfinite(t["deviance"].sum())
    assert best[0] >= 10 and best[1] >= 100


@pytest.mark.parametrize("name,mode", [("P4", "mixed"), ("P4", "mixed_f32"), ("P4", "fp64"),
                                       ("P100", "mixed")])
def test_steep_designs_on_the_emulator(name, mode):
    """The Newton emulator ends "ok" without an escalation or a halving (P =
    100: the first partition, the affordable one)."""
    X, y, off, ref = _steep(name)
    parts = range(len(off) - 1) if name == "P4" else (0,)
    for k in parts:
        a, b = off[k], off[k + 1]
        tr = N.trajectory(X[a:b], y[a:b], fit_intercept=True, mode=mode, max_iter=100)
        assert tr["status"] == "ok" and tr["iters"] < 50, (name, k, tr["status"], tr["iters"])
        assert not any(r["escalated"] or r["halved"] for r in tr["rec"]), (name, k)
        assert np.abs(tr["final"] - ref["theta"][k]).max() <= 1e-8 * np.abs(ref["theta"][k]).max()
