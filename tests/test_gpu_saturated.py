"""GPU: the GLM row terms at saturated linear predictors, against the
long-double yardstick tests/_sat_ref.py (pinned on the CPU by
tests/test_cpu_saturated.py, which also asserts the steep designs'
preconditions).

**Row level.**  One-row partitions (``offsets`` steps of 1), so every output
entry is one row's term, with a 33-row partition of ordinary data after every
15 of them (block tails and neighbours).  eta is posed exactly: p = 1 without
an intercept, beta = [1], X[:, 0] = eta; for the Poisson family also through
``eta_offset`` (X = 0 in the evaluation passes; X = 1 and beta = [0] in the
score pass, whose gram is then d and whose score is s); once through ``center``
/ ``scale`` with scale = 1/8; on the code layout as x + c with one numeric
column and one two-level factor, both coefficients 1.  The grid is both signs
of ``_sat_ref.GRID``: the logistic y in {0, 1} everywhere and the grouped y =
0.25 (weight 4) at |eta| >= 20; the Poisson y in {0, 1, 3, 351} on [-800, 709]
and at the overflow rows eta = 710, 800.  Every input is a finite number; the
infinite outputs are ordinary arithmetic.

**Bounds** (``_sat_ref``; eps = 2^-53), from the operation and not from the
code under test: log-likelihood 8 eps omega max(1, |eta|) (logistic), 8 eps
omega (|y eta| + mu + |lgamma(y + 1)|) (Poisson); deviance twice that plus 8 eps
omega |saturated term|; Pearson and the information's w by the class of the
reference value (relative 1e-12, plus 4 * 4.94e-324 / ea where ea is
subnormal; below 2^-1022: |got| <= 2^-1000 omega; above 2^1022: that or +inf;
infinite: exactly); the score's s within 4 eps omega + 1e-12 |s|, hence its
square within (2 |s| d + d^2) + 1e-12 s^2, d = 4 eps omega.  A multi-row
partition is held to 1e-12 |ref_k| + the sum of its rows' bounds.  No output
is NaN.  Every call runs twice, bit for bit.  Each test prints the worst ratio
to its bound before it asserts.  (The subnormal band 708 < |eta| < 745.13 holds
as stated: the device exp returns rounded subnormals, it does not flush.)

**Sum level.**  The steep designs of ``_sat_ref.steep_design`` (half the rows
x0 ~ U(-1, 1), half U(-130, 130), slope 6): fits against ``_glm_ref.fit`` at
the project's 1e-8 / 1e-10, then the evaluation, goodness-of-fit and score
passes at each fit's own theta and at perturbed candidates against the
long-double sums, the ragged sizes (1000, 31, 0, 2049) appended.
"""

import functools

import numpy as np
import pytest

import _glm_ref as G
import _gof_ref as R
import _sat_ref as S
from test_gpu_gof import FAMILY_MASKS, FM_IDS

pytestmark = pytest.mark.gpu

LD = S.LD
FILLER, EVERY = 33, 15


@pytest.fixture(scope="module")
def M():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a visible MI355X"
    from dlsa_amd import models
    return models


def _host(g):
    return {k: v.cpu().numpy() for k, v in g.items()}


def _twice(fn):
    """The call's result (a tensor, a tuple or a dict of tensors) as numpy,
    after a second call gave the same bits."""
    import torch

    def flat(r):
        return list(r.values()) if isinstance(r, dict) else list(r) if isinstance(r, tuple) else [r]

    a, b = fn(), fn()
    for u, v in zip(flat(a), flat(b)):
        assert torch.equal(u, v) or (u.dtype.is_floating_point and
                                     u.cpu().numpy().tobytes() == v.cpu().numpy().tobytes()), \
            "two calls differ"
    if isinstance(a, dict):
        return _host(a)
    return tuple(t.cpu().numpy() for t in a) if isinstance(a, tuple) else a.cpu().numpy()


# ---- the posed rows --------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _posed(family, weighted):
    """y, eta, omega, offsets of the grid's rows as one-row partitions with a
    33-row partition of ordinary data (eta multiples of 2^-10 in [-3, 3]) after
    every 15; ``one``: the partitions of one posed row.  Weighted: the grouped
    rows keep their 4, the others cycle through (1, 0.5, 3); the ordinary rows
    take U(0.2, 5) with zeros.  Unweighted: omega = 1 everywhere."""
    y, eta, om = S.grid_rows(family)
    if weighted:
        om = np.where(om == 1.0, np.tile([1.0, 0.5, 3.0], len(om))[:len(om)], om)
    else:
        om = np.ones(len(om))
    rng = np.random.default_rng(5)
    ys, es, oms, sizes, one = [], [], [], [], []
    for i in range(0, len(y), EVERY):
        j = min(i + EVERY, len(y))
        ys.append(y[i:j]), es.append(eta[i:j]), oms.append(om[i:j])
        sizes += [1] * (j - i)
        one += [True] * (j - i)
        ef = np.round(rng.uniform(-3, 3, FILLER) * 1024) / 1024
        if family == "logistic":
            yf = (rng.uniform(size=FILLER) < G._expit(ef)).astype(np.float64)
        else:
            yf = rng.poisson(np.exp(ef)).astype(np.float64)
        wf = G.weights(FILLER, "real", seed=i) if weighted else np.ones(FILLER)
        ys.append(yf), es.append(ef), oms.append(wf)
        sizes.append(FILLER)
        one.append(False)
    out = dict(y=np.concatenate(ys), eta=np.concatenate(es), om=np.concatenate(oms),
               off=S.offsets_of(sizes), one=np.array(one))
    for v in out.values():
        v.setflags(write=False)
    return out


def _sums(rows_ld, off):
    """The partitions' long-double sums of the rows' values, rounded once."""
    out = np.zeros(len(off) - 1, dtype=LD)
    with np.errstate(over="ignore", invalid="ignore"):
        for k, (a, b) in enumerate(zip(off[:-1], off[1:])):
            out[k] = rows_ld[a:b].sum(dtype=LD) if b > a else LD(0)
    return S.to64(out)


def _bsum(rows, off):
    """The partitions' sums of the rows' (fp64) bounds."""
    return np.array([rows[a:b].sum() for a, b in zip(off[:-1], off[1:])])


def _ratio(got, ref, bound, off, what):
    """Worst |got - ref| over (bound, plus 1e-12 |ref| on a partition of more
    than one row); a reference above 2^1022 also passes by its infinity, an
    infinite one only by it, a NaN nowhere.  Prints, then returns the ratios."""
    got, ref = np.asarray(got, np.float64).reshape(-1), np.asarray(ref, np.float64)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    many = np.diff(off) > 1
    with np.errstate(invalid="ignore", over="ignore"):
        b = bound + np.where(many & np.isfinite(ref), S.REL * np.abs(ref), 0.0)
    r = S.abs_ratio(got, ref, b)
    same_inf = np.isinf(got) & (np.sign(got) == np.sign(ref))
    r = np.where((np.abs(ref) > S.HUGE) & same_inf, 0.0, r)
    k = int(np.argmax(r))
    print(f"{what}: worst ratio to the bound {r[k]:.3g} (partition {k}: got {got[k]!r} ref "
          f"{ref[k]!r}); NaN entries: {int(np.isnan(got).sum())}")
    return r


def _assert(r, what, d=None):
    bad = np.nonzero(~(r <= 1.0))[0]
    rows = "" if d is None else [(float(d["y"][d["off"][k]]), float(d["eta"][d["off"][k]]))
                                 for k in bad[:10]]
    assert bad.size == 0, (what, f"{bad.size} partitions past the bound", bad[:10].tolist(),
                           "their first rows' (y, eta)", rows)


def _refs(family, d):
    """Per partition: the reference values and bounds of the row terms."""
    y, eta, om, off = d["y"], d["eta"], d["om"], d["off"]
    t = S.row_terms_ld(family, y, eta, om)
    r64 = S.row_terms(family, y, eta, om)
    x2 = np.asarray(eta, LD) ** 2
    out = {
        "loglik": (_sums(t["loglik"], off), _bsum(S.loglik_bound(family, y, eta, om), off)),
        "deviance": (_sums(t["deviance"], off), _bsum(S.deviance_bound(family, y, eta, om), off)),
        "pearson": (_sums(t["pearson"], off),
                    _bsum(S.class_bound(r64["pearson"], r64["tiny"], om), off)),
        # the score pass with x = eta: gram = d x^2, score = s x
        "info_x": (_sums(t["w"] * x2, off),
                   _bsum(S.class_bound(S.to64(t["w"] * x2), r64["tiny"], om), off)),
        "meat_x": (_sums(t["s"] * t["s"] * x2, off),
                   _bsum(S.score_sq_bound(r64["s"], om) * eta ** 2, off)),
        "score_x": (_sums(t["s"] * np.asarray(eta, LD), off),
                    _bsum(S.score_bound(r64["s"], om) * np.abs(eta), off)),
        # and with x = 1 (eta through the offset): gram = d, score = s
        "info_1": (_sums(t["w"], off), _bsum(S.class_bound(r64["w"], r64["tiny"], om), off)),
        "meat_1": (_sums(t["s"] * t["s"], off), _bsum(S.score_sq_bound(r64["s"], om), off)),
        "score_1": (_sums(t["s"], off), _bsum(S.score_bound(r64["s"], om), off)),
    }
    return out


def _pose(d, how):
    """X [n, 1], beta, eta_offset, center, scale that give eta exactly."""
    eta = d["eta"]
    if how == "x":
        return eta[:, None].copy(), np.array([1.0]), None, None, None
    if how == "ofs":
        return np.zeros((len(eta), 1)), np.array([1.0]), eta.copy(), None, None
    assert how == "std"  # (x - 1024) * 8 with x = eta / 8 + 1024, exact on the grid
    x = eta / 8.0 + 1024.0
    assert ((x - 1024.0) * 8.0 == eta).all()
    return x[:, None].copy(), np.array([1.0]), None, np.array([1024.0]), np.array([0.125])


# ---- row level: the evaluation passes ------------------------------------------------------------

LOGLIK_CASES = [("logistic", False, "x"), ("logistic", True, "x"), ("logistic", True, "std"),
                ("poisson", False, "x"), ("poisson", False, "ofs"), ("poisson", True, "x"),
                ("poisson", True, "ofs"), ("poisson", False, "std")]


@pytest.mark.parametrize("family,weighted,how", LOGLIK_CASES,
                         ids=[f"{f}-{'wgt' if w else 'none'}-{h}" for f, w, h in LOGLIK_CASES])
def test_loglik_rows(M, family, weighted, how):
    """``logistic_loglik_batched`` (with and without weights), ``poisson_loglik_batched``,
    ``_offset`` and ``_weighted``."""
    d = _posed(family, weighted)
    X, beta, o, c, s = _pose(d, how)
    kw = dict(center=c, scale=s)
    w = d["om"] if weighted else None
    if family == "logistic":
        fn = lambda: M.logistic_loglik_batched(X, d["y"], d["off"], beta[None], sample_weight=w, **kw)
    elif weighted:
        fn = lambda: M.poisson_loglik_batched_weighted(X, d["y"], d["off"], beta[None],
                                                       sample_weight=w, eta_offset=o, **kw)
    elif how == "ofs":
        fn = lambda: M.poisson_loglik_batched_offset(X, d["y"], d["off"], beta[None], eta_offset=o)
    else:
        fn = lambda: M.poisson_loglik_batched(X, d["y"], d["off"], beta[None], **kw)
    got = _twice(fn)
    ref, bound = _refs(family, d)["loglik"]
    what = f"loglik {family} weighted={weighted} {how}"
    _assert(_ratio(got, ref, bound, d["off"], what), what, d)


# the masks with an offset pose eta through it; the others through X, plain and standardised
GOF_CASES = [(fm, how) for fm in FAMILY_MASKS
             for how in (("ofs",) if fm[1] in ("ofs", "both") else ("x", "std"))]


@pytest.mark.parametrize("fm,how", GOF_CASES, ids=[f"{f}-{m}-{h}" for (f, m), h in GOF_CASES])
def test_gof_rows(M, fm, how):
    """``glm_gof_batched``, both families and every extras mask.  Fails on the kernels of before the fix at
    the matched logistic rows y = 1, eta >= 37 (0 for exp(-eta)), at every row
    whose exp(-|eta|) is 0 (NaN), at the Poisson y = 0 rows over an underflowed
    mu (NaN), at the overflow rows (NaN) and at eta >= 500, where (y - mu)^2
    overflowed."""
    family, mask = fm
    weighted = mask in ("wgt", "both")
    d = _posed(family, weighted)
    X, beta, o, c, s = _pose(d, how)
    got = _twice(lambda: M.glm_gof_batched(family, X, d["y"], d["off"], betas=beta[None],
                                           eta_offset=o, sample_weight=d["om"] if weighted else None,
                                           center=c, scale=s, return_sum=False))
    refs = _refs(family, d)
    assert got["n_pos"].tolist() == [int((d["om"][a:b] > 0).sum())
                                     for a, b in zip(d["off"][:-1], d["off"][1:])]
    bad = []
    for name in ("deviance", "pearson"):
        what = f"gof {family}-{mask} {how} {name}"
        bad.append((_ratio(got[name], *refs[name], d["off"], what), what))
    for r, what in bad:
        _assert(r, what, d)


@pytest.mark.parametrize("kind", ["score", "information"])
@pytest.mark.parametrize("fm", FAMILY_MASKS, ids=FM_IDS)
def test_gram_rows(M, fm, kind):
    """``glm_gram_batched`` with P = 1: gram = d x^2 and score = s x with x =
    eta, or d and s with x = 1 and eta through the offset."""
    family, mask = fm
    weighted = mask in ("wgt", "both")
    d = _posed(family, weighted)
    refs = _refs(family, d)
    if mask in ("ofs", "both"):
        X, beta, o, tag = np.ones((len(d["y"]), 1)), np.array([0.0]), d["eta"].copy(), "1"
    else:
        X, beta, o, tag = d["eta"][:, None].copy(), np.array([1.0]), None, "x"
    got = _twice(lambda: M.glm_gram_batched(family, X, d["y"], d["off"], beta=beta, kind=kind,
                                            eta_offset=o,
                                            sample_weight=d["om"] if weighted else None))
    what = f"gram {family}-{mask} {kind}"
    gname = ("meat_" if kind == "score" else "info_") + tag
    # eta = 0 with x = eta is a row of zeros: 0 * d, which is NaN only where d is infinite
    rg = _ratio(got["gram"], *refs[gname], d["off"], what + " gram")
    rs = _ratio(got["score"], *refs["score_" + tag], d["off"], what + " score")
    _assert(rg, what + " gram", d)
    _assert(rs, what + " score", d)


# ---- row level: the code layout ------------------------------------------------------------------

def _codes(d):
    """One numeric column and one two-level factor, coefficients (1, 1): eta =
    x + c with c the row's code, x = eta - c exact on the grid."""
    code = (np.arange(len(d["eta"])) % 2).astype(np.uint8)
    x = d["eta"] - code
    assert (x + code == d["eta"]).all()
    return x[:, None].copy(), code[:, None].copy(), [2], np.array([[1.0, 1.0]])


@pytest.mark.parametrize("fm", [("logistic", "none"), ("logistic", "wgt"), ("poisson", "none"),
                                ("poisson", "wgt")], ids=["logistic-none", "logistic-wgt",
                                                          "poisson-none", "poisson-wgt"])
def test_code_layout_rows(M, fm):
    """``logistic_loglik_batched_categorical``, ``poisson_loglik_batched_categorical``
    and ``glm_gof_batched_categorical``."""
    family, mask = fm
    weighted = mask == "wgt"
    d = _posed(family, weighted)
    Xn, codes, levels, betas = _codes(d)
    w = d["om"] if weighted else None
    ll_fn = M.logistic_loglik_batched_categorical if family == "logistic" else \
        M.poisson_loglik_batched_categorical
    ll = _twice(lambda: ll_fn(Xn, codes, d["y"], d["off"], levels, betas, sample_weight=w))
    g = _twice(lambda: M.glm_gof_batched_categorical(family, Xn, codes, d["y"], d["off"], levels,
                                                     betas=betas, sample_weight=w))
    refs = _refs(family, d)
    res = []
    for name, got in (("loglik", ll), ("deviance", g["deviance"]), ("pearson", g["pearson"])):
        what = f"codes {family}-{mask} {name}"
        res.append((_ratio(got, *refs[name], d["off"], what), what))
    for r, what in res:
        _assert(r, what, d)


# ---- sum level: the steep designs ----------------------------------------------------------------

RAGGED = (1000, 31, 0, 2049)
FIT_REL = 1e-8


@functools.lru_cache(maxsize=None)
def _steep(name, weighted=False):
    """X, y, offsets, weights and the reference fits of one steep case."""
    p, sizes, seed = S.STEEP[name]
    off = S.offsets_of(sizes)
    X, y, _ = S.steep_design(int(off[-1]), p, seed)
    w = G.weights(len(y), "real") if weighted else None
    ref = G.fit_partitions("logistic", X, y, off, w=w, fit_intercept=True)
    return X, y, off, w, ref


def _rel(a, b):
    return float(np.abs(np.asarray(a) - np.asarray(b)).max() / np.abs(np.asarray(b)).max())


def _check_fit(fit, ref, what, status=None):
    st = fit.status.cpu().numpy()
    K = len(st)
    assert st.tolist() == (status or [0] * K), (what, fit.status_counts())
    th, S_, St, ll = (getattr(fit, k).cpu().numpy() for k in ("theta", "sig_inv", "sig_inv_theta",
                                                                "loglik"))
    for k in range(K):
        if st[k] != 0:
            continue
        figs = (_rel(th[k], ref["theta"][k]), _rel(S_[k], ref["sig_inv"][k]),
                _rel(St[k], ref["sig_inv_theta"][k]),
                abs(ll[k] - ref["loglik"][k]) / abs(ref["loglik"][k]))
        print(f"{what} partition {k}: theta {figs[0]:.2e} sig_inv {figs[1]:.2e} sig_inv_theta "
              f"{figs[2]:.2e} loglik {figs[3]:.2e} iters {int(fit.iters[k])} (reference "
              f"{int(ref['iters'][k])})")
        assert max(figs[:3]) <= FIT_REL and figs[3] <= 1e-10, (what, k, figs)


def _fit_twice(fn):
    import torch

    a, b = fn(), fn()
    for k in ("theta", "sig_inv", "sig_inv_theta", "loglik", "iters", "status"):
        u, v = getattr(a, k), getattr(b, k)
        assert u.cpu().numpy().tobytes() == v.cpu().numpy().tobytes(), ("two fits differ", k)
    return a


def _sum_refs(family, Z, y, off, coef_of, w=None, o=None, mats_too=True):
    """Per partition (its coefficient vector ``coef_of(k)``) the long-double
    sums and bounds of loglik, deviance, Pearson, the information and meat
    matrices and the score vector."""
    K, P = len(off) - 1, Z.shape[1]
    out = {k: np.zeros(K) for k in ("loglik", "deviance", "pearson")}
    bnd = {k: np.zeros(K) for k in out}
    mats = {k: np.zeros((K, P, P)) for k in ("information", "score")}
    mbnd = {k: np.zeros((K, P, P)) for k in mats}
    vec, vbnd = np.zeros((K, P)), np.zeros((K, P))
    for k, (a, b) in enumerate(zip(off[:-1], off[1:])):
        if b == a:
            continue
        yk, Zk = y[a:b], Z[a:b]
        wk = None if w is None else w[a:b]
        om = np.ones(b - a) if w is None else wk
        eta = S.eta_ld(Zk, coef_of(k), None if o is None else o[a:b])
        e64 = S.to64(eta)
        t = S.row_terms_ld(family, yk, eta, wk)
        r64 = {n: S.to64(t[n]) for n in S.KEYS + ("tiny",)}
        assert np.isfinite(r64["pearson"]).all() and np.isfinite(r64["deviance"]).all(), \
            "the sum-level cases have no infinite row"
        rows = {"loglik": S.loglik_bound(family, yk, e64, wk),
                "deviance": S.deviance_bound(family, yk, e64, wk),
                "pearson": S.class_bound(r64["pearson"], r64["tiny"], om)}
        for n in out:
            out[n][k] = float(t[n].sum(dtype=LD))
            bnd[n][k] = S.REL * abs(out[n][k]) + rows[n].sum()
        if not mats_too:
            continue
        Zl, Za = Zk.astype(LD), np.abs(Zk)
        for n, dl, db in (("information", t["w"], S.class_bound(r64["w"], r64["tiny"], om)),
                          ("score", t["s"] * t["s"], S.score_sq_bound(r64["s"], om))):
            mats[n][k] = S.to64(Zl.T @ (Zl * dl[:, None]))
            mbnd[n][k] = S.REL * np.abs(mats[n][k]) + Za.T @ (Za * db[:, None])
        vec[k] = S.to64(Zl.T @ t["s"])
        vbnd[k] = S.REL * np.abs(vec[k]) + Za.T @ S.score_bound(r64["s"], om)
    return out, bnd, mats, mbnd, vec, vbnd


def _worst(got, ref, bound, what):
    with np.errstate(invalid="ignore", divide="ignore"):
        r = np.where(got == ref, 0.0, np.abs(got - ref) / np.where(bound > 0, bound, 1.0))
        r = np.where((bound == 0) & (got != ref), np.inf, r)
    r = np.where(np.isnan(got), np.inf, r)
    print(f"{what}: worst ratio to the bound {float(r.max(initial=0.0)):.3g}")
    return float(r.max(initial=0.0))


def _sum_checks(M, family, X, y, off, thetas, what, w=None, o=None, sig_inv=None, gram=True):
    """The evaluation, goodness-of-fit and score passes at ``thetas`` [K, P]
    (each partition at its own row) and at two perturbed shared candidates,
    with the ragged partitions appended (they take partition 0's theta)."""
    rng = np.random.default_rng(9)
    n0, K0 = int(off[-1]), len(off) - 1
    extra = sum(RAGGED)
    Xa = np.concatenate([X, X[:extra]])
    ya = np.concatenate([y, y[:extra]])
    wa = None if w is None else np.concatenate([w, w[:extra]])
    oa = None if o is None else np.concatenate([o, o[:extra]])
    offa = np.concatenate([off, n0 + np.cumsum(RAGGED)]).astype(np.int64)
    th = np.concatenate([thetas, np.repeat(thetas[:1], len(RAGGED), 0)])
    Z = G.design(Xa, True)
    P = Z.shape[1]
    betas = thetas[0] * np.array([[0.97], [1.02]]) + rng.standard_normal((2, P)) * 0.01
    kw = dict(fit_intercept=True)
    ekw = dict(kw, sample_weight=wa) if family == "logistic" else \
        dict(kw, sample_weight=wa, eta_offset=oa)
    ll_fn = M.logistic_loglik_batched if family == "logistic" else M.poisson_loglik_batched_weighted
    worst = []
    # each partition at its own theta
    ref, bnd, mats, mbnd, vec, vbnd = _sum_refs(family, Z, ya, offa, lambda k: th[k], wa, oa)
    g = _twice(lambda: M.glm_gof_batched(family, Xa, ya, offa, thetas=th, eta_offset=oa,
                                         sample_weight=wa, **kw))
    for n in ("deviance", "pearson"):
        worst.append(_worst(g[n][:, 0], ref[n], bnd[n], f"{what} own theta {n}"))
    if gram:
        for kind in ("information", "score"):
            gg = _twice(lambda: M.glm_gram_batched(family, Xa, ya, offa, thetas=th, kind=kind,
                                                   eta_offset=oa, sample_weight=wa, **kw))
            worst.append(_worst(gg["gram"], mats[kind], mbnd[kind], f"{what} own theta {kind}"))
            worst.append(_worst(gg["score"], vec, vbnd, f"{what} own theta {kind} score"))
            if kind == "information" and sig_inv is not None:
                for k in range(K0):
                    e = _rel(gg["gram"][k], sig_inv[k])
                    print(f"{what} partition {k}: information vs sig_inv {e:.2e}")
                    assert e <= FIT_REL, (what, k, e)
    # the shared candidates (the log-likelihood pass takes only those)
    ll = _twice(lambda: ll_fn(Xa, ya, offa, np.concatenate([th[:1], betas]), **ekw))
    gb = _twice(lambda: M.glm_gof_batched(family, Xa, ya, offa, betas=betas, eta_offset=oa,
                                          sample_weight=wa, **kw))
    for j, b in enumerate([th[0]] + list(betas)):
        ref, bnd, mats, mbnd, vec, vbnd = _sum_refs(family, Z, ya, offa, lambda k: b, wa, oa,
                                                    mats_too=gram and j == 1)
        worst.append(_worst(ll[:, j], ref["loglik"], bnd["loglik"], f"{what} beta {j} loglik"))
        if j == 0:
            continue
        for n in ("deviance", "pearson"):
            worst.append(_worst(gb[n][:, j - 1], ref[n], bnd[n], f"{what} beta {j} {n}"))
        if gram and j == 1:
            for kind in ("information", "score"):
                gg = _twice(lambda: M.glm_gram_batched(family, Xa, ya, offa, beta=b, kind=kind,
                                                       eta_offset=oa, sample_weight=wa, **kw))
                worst.append(_worst(gg["gram"], mats[kind], mbnd[kind], f"{what} beta {kind}"))
                worst.append(_worst(gg["score"], vec, vbnd, f"{what} beta {kind} score"))
    assert max(worst) <= 1.0, (what, worst)


STEEP_FITS = [("P4", "mixed"), ("P4", "mixed_f32"), ("P4", "fp64"), ("P100", "mixed"),
              ("P100", "mixed_f32"), ("P132", "fp64")]


@pytest.mark.parametrize("name,mode", STEEP_FITS, ids=[f"{n}-{m}" for n, m in STEEP_FITS])
def test_steep_logistic_fit_and_sums(M, name, mode):
    """The fit against ``_glm_ref.fit`` with every partition ok and no fp32
    escalation (the emulator shows none: tests/test_cpu_saturated.py), twice
    bit for bit; then the sums at its theta (once per shape, in its first
    mode)."""
    X, y, off, _, ref = _steep(name)
    fit = _fit_twice(lambda: M.logistic_model_batched(X, y, off, fit_intercept=True, hessian=mode))
    print(name, mode, {k: fit.stats[k] for k in ("iterations", "passes_fp32", "passes_f32x",
                                                 "passes_fp64", "passes_oz")})
    _check_fit(fit, ref, f"steep {name} {mode}")
    assert fit.stats["passes_f32x"] == 0
    if mode == [m for n, m in STEEP_FITS if n == name][0]:
        _sum_checks(M, "logistic", X, y, off, fit.theta.cpu().numpy(), f"steep {name}",
                    sig_inv=fit.sig_inv.cpu().numpy())


def test_steep_weighted_logistic_fit_and_sums(M):
    X, y, off, w, ref = _steep("P4", True)
    fit = _fit_twice(lambda: M.logistic_model_batched_weighted(X, y, off, sample_weight=w,
                                                               fit_intercept=True))
    _check_fit(fit, ref, "steep weighted P4")
    assert fit.stats["passes_f32x"] == 0
    _sum_checks(M, "logistic", X, y, off, fit.theta.cpu().numpy(), "steep weighted P4", w=w,
                sig_inv=fit.sig_inv.cpu().numpy())


def test_steep_code_layout_fit_and_sums(M):
    """q = 2 numeric columns, the steep one first, and one four-level factor
    (P = 6 with the intercept), against the reference fit of the expanded
    design; the evaluation and goodness-of-fit passes of the code layout at the
    fit's thetas against the long-double sums."""
    import torch

    sizes = (2000, 1500)
    off = S.offsets_of(sizes)
    n = int(off[-1])
    X, _, _ = S.steep_design(n, 2, 4)
    rng = np.random.default_rng(14)
    codes = rng.integers(0, 4, (n, 1)).astype(np.uint8)
    levels = [4]
    Xd = M.expand_categorical(torch.from_numpy(X), torch.from_numpy(codes), levels).numpy()
    theta = np.array([0.3, 6.0, -0.7, 0.5, -0.4, 0.8])
    Z = G.design(Xd, True)
    with np.errstate(over="ignore"):
        y = (rng.uniform(size=n) < G._expit(Z @ theta)).astype(np.float64)
    ref = G.fit_partitions("logistic", Xd, y, off, fit_intercept=True)
    assert (ref["iters"] < 50).all() and max(np.linalg.cond(s) for s in ref["sig_inv"]) < 1e3
    fit = _fit_twice(lambda: M.logistic_model_batched_categorical(X, codes, y, off, levels,
                                                                  fit_intercept=True))
    _check_fit(fit, ref, "steep codes")
    th = fit.theta.cpu().numpy()
    ae = np.abs(Z[:sizes[0]] @ th[0])
    assert (ae > 745.13).sum() >= 10 and ((ae > 40) & (ae < 700)).sum() >= 100
    r, bnd, *_ = _sum_refs("logistic", Z, y, off, lambda k: th[k], mats_too=False)
    g = _twice(lambda: M.glm_gof_batched_categorical("logistic", X, codes, y, off, levels,
                                                     thetas=th, fit_intercept=True))
    worst = [_worst(g[n_][:, 0], r[n_], bnd[n_], f"steep codes {n_}")
             for n_ in ("deviance", "pearson")]
    ll = _twice(lambda: M.logistic_loglik_batched_categorical(X, codes, y, off, levels, th[:1],
                                                              fit_intercept=True))
    r0, b0, *_ = _sum_refs("logistic", Z, y, off, lambda k: th[0], mats_too=False)
    worst.append(_worst(ll[:, 0], r0["loglik"], b0["loglik"], "steep codes loglik"))
    assert max(worst) <= 1.0, worst


@functools.lru_cache(maxsize=None)
def _dead_rows(p, sizes, seed):
    """An ordinary Poisson design (X ~ U(-1, 1), log exposure ~ U(log 0.2, log
    5), coefficients U(-1, 1) / sqrt(p), intercept 0.5) with weights and,
    appended to every partition, 200 dead rows: y = 0 and o in {-720, -745, -746, -800}
    (mu subnormal or 0)."""
    rng = np.random.default_rng(seed)
    theta = np.concatenate([[0.5], rng.uniform(-1, 1, p) / np.sqrt(p)])
    Xs, ys, os_, out_sizes = [], [], [], []
    for m in sizes:
        Xk = rng.uniform(-1, 1, (m, p))
        ok = rng.uniform(np.log(0.2), np.log(5.0), m)
        yk = rng.poisson(np.exp(Xk @ theta[1:] + theta[0] + ok)).astype(np.float64)
        dead = np.tile([-720.0, -745.0, -746.0, -800.0], 50)
        Xs += [Xk, rng.uniform(-1, 1, (200, p))]
        ys += [yk, np.zeros(200)]
        os_ += [ok, dead]
        out_sizes.append(m + 200)
    X, y, o = np.concatenate(Xs), np.concatenate(ys), np.concatenate(os_)
    off = S.offsets_of(out_sizes)
    w = G.weights(len(y), "real")
    ref = G.fit_partitions("poisson", X, y, off, w=w, o=o, fit_intercept=True)
    return np.ascontiguousarray(X), y, o, w, off, ref


@pytest.mark.parametrize("p,sizes", [(3, (1800, 400, 1800)), (99, (2801, 2801))], ids=["P4", "P100"])
def test_poisson_dead_rows_fit_and_sums(M, p, sizes):
    X, y, o, w, off, ref = _dead_rows(p, sizes, 17)
    assert (ref["iters"] < 50).all() and np.isfinite(ref["theta"]).all()
    fit = _fit_twice(lambda: M.poisson_model_batched_weighted(X, y, off, sample_weight=w,
                                                              eta_offset=o, fit_intercept=True))
    _check_fit(fit, ref, f"dead rows P={p + 1}")
    _sum_checks(M, "poisson", X, y, off, fit.theta.cpu().numpy(), f"dead rows P={p + 1}", w=w, o=o,
                sig_inv=fit.sig_inv.cpu().numpy())


def test_steep_job_hc0_and_dispersion(M):
    """``dlsa_fit_sharded`` on the steep P = 4 case: cov_type="HC0" gives finite
    standard errors, dispersion="pearson" a finite phi that is
    ``_gof_ref.dispersion`` fed from the long-double Pearson sums within 1e-10."""
    from dlsa_amd.distributed import dlsa_fit_sharded

    X, y, off, _, _ = _steep("P4")
    hc0 = dlsa_fit_sharded(X, y, off, fit_intercept=True, cov_type="HC0")
    assert np.isfinite(hc0["std_err"]).all() and (hc0["std_err"] > 0).all()
    out = dlsa_fit_sharded(X, y, off, fit_intercept=True, dispersion="pearson")
    fit = out["fit"]
    th, st = fit.theta.cpu().numpy(), fit.status.cpu().numpy()
    assert (st == 0).all()
    Z = G.design(X, True)
    r, *_ = _sum_refs("logistic", Z, y, off, lambda k: th[k], mats_too=False)
    phi = R.dispersion(r["pearson"], np.diff(off), fit.P)
    print(f"dispersion {out['dispersion']!r} yardstick {phi!r}")
    assert np.isfinite(out["dispersion"]) and abs(out["dispersion"] / phi - 1.0) <= 1e-10
