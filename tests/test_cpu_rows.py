"""CPU: the yardstick of the row diagnostics pass (tests/_rows_ref.py) pinned
against the hat matrix, the goodness-of-fit sums and a long-double evaluation;
the Python surface and the C entry's argument checks; ``rows_factor``; and the
HC3 path of ``dlsa_fit_sharded`` on stubbed passes."""

import ctypes
import inspect

import numpy as np
import pytest

import _glm_ref as G
import _gof_ref as GOF
import _gram_ref as GR
import _rows_ref as RR
import _sat_ref as SAT

CASES = [("logistic", False, False), ("logistic", True, False), ("poisson", False, False),
         ("poisson", True, False), ("poisson", True, True)]
CASE_IDS = ["logistic", "logistic-wgt", "poisson", "poisson-wgt", "poisson-wgt-ofs"]


def _small(family, wgt, ofs, n=40, p=3):
    rng = np.random.default_rng(5)
    Z = G.design(rng.standard_normal((n, p)) * 0.6, True)
    theta = np.array([0.3, 0.5, -0.4, 0.2])
    o = rng.uniform(np.log(0.5), np.log(2.0), n) if ofs else None
    eta = Z @ theta + (0.0 if o is None else o)
    y = (rng.poisson(np.exp(eta)) if family == "poisson"
         else (rng.uniform(size=n) < G._expit(eta))).astype(np.float64)
    w = G.weights(n, "real") if wgt else None
    return Z, y, theta + 0.1, w, o


# ---- the yardstick ----------------------------------------------------------------------------

@pytest.mark.parametrize("family,wgt,ofs", CASES, ids=CASE_IDS)
def test_leverage_is_the_diagonal_of_the_hat_matrix(family, wgt, ofs):
    Z, y, theta, w, o = _small(family, wgt, ofs)
    S = RR.information(family, Z, theta, w, o)
    assert np.abs(S - G.hessian(family, Z, theta, w, o)).max() <= 1e-13 * np.abs(S).max()
    r = RR.rows(family, Z, y, theta, RR.factor(S), w, o)
    sw = np.sqrt(r["d"])
    H = (Z * sw[:, None]) @ np.linalg.inv(S) @ (Z * sw[:, None]).T
    assert np.abs(r["leverage"] - np.diag(H)).max() <= 1e-12
    assert abs(r["leverage"].sum() - Z.shape[1]) <= 1e-12 * Z.shape[1]
    assert (r["leverage"] >= 0).all() and (r["leverage"] < 1).all()


@pytest.mark.parametrize("family,wgt,ofs", CASES, ids=CASE_IDS)
def test_squared_residuals_sum_to_the_goodness_of_fit(family, wgt, ofs):
    Z, y, theta, w, o = _small(family, wgt, ofs)
    r = RR.rows(family, Z, y, theta, None, w, o)
    dev, chi, _ = GOF.gof(family, Z, y, theta, w, o)
    assert abs((r["dev_res"] ** 2).sum() - dev) <= 1e-12 * dev
    assert abs((r["pearson_res"] ** 2).sum() - chi) <= 1e-10 * chi
    for name in ("dev_res", "pearson_res"):  # (a row of weight 0 is a signed zero)
        assert np.array_equal(np.signbit(r[name]), y - r["mu"] < 0), name


LD_CASES = [(15, True, "logistic", "wgt"), (15, True, "poisson", "both"),
            (33, False, "logistic", "none"), (33, False, "poisson", "ofs"),
            (100, True, "logistic", "wgt"), (100, True, "poisson", "both")]


@pytest.mark.parametrize("p,fi,family,mask", LD_CASES,
                         ids=[f"p{p}-{f}-{m}" for p, _, f, m in LD_CASES])
def test_fp64_yardstick_against_long_double(p, fi, family, mask):
    """On the GPU test's inputs: fp64 numpy within a quarter of every bound of
    the long-double evaluation; sum h = P per partition with R from the
    information at the same theta; fewer than 1 % of the Poisson rows, and no
    0/1 logistic row, of positive weight under the sign check's bound."""
    d = RR.dense(p, fi)
    o, w = RR.extras(d, mask)
    y, off, Z, P = d[family], d["off"], d["Z"], p + fi
    S = RR.own_factors(family, Z, off, d["thetas"], w, o)
    R = np.stack([RR.factor(S[k]) if k != RR.EMPTY else np.full((P, P), np.nan)
                  for k in range(len(S))])
    for k in (0, 1, 3, 5):
        a, b = int(off[k]), int(off[k + 1])
        args = (family, Z[a:b], y[a:b], d["thetas"][k])
        kw = dict(w=None if w is None else w[a:b], o=None if o is None else o[a:b])
        ref = RR.rows(*args, R=R[k], **kw)
        bnd = RR.bounds(*args, ref=ref, R=R[k], **kw)
        ld = RR.rows_ld(*args, R=R[k], **kw)
        for name, key in (("eta", "eta"), ("mu", "mu"), ("dev", "dev"), ("chi", "chi"),
                          ("leverage", "leverage")):
            err = SAT.to64(np.abs(np.asarray(ref[key], SAT.LD) - ld[key]))
            ratio = float(RR.ratio(err, bnd[name]).max())
            print(f"p={p} {family}-{mask} k={k} {name}: {ratio:.3f} of the bound")
            assert ratio <= 0.25, (name, k, ratio)
        assert abs(ref["leverage"].sum() - P) <= 1e-9 * P
        assert (ref["leverage"] >= 0).all() and (ref["leverage"] < 1).all()
        pos = np.ones(b - a, bool) if w is None else w[a:b] > 0  # (weight 0: a signed zero)
        weak_d = pos & (np.abs(ref["dev"]) <= bnd["dev"])
        weak_c = pos & (np.abs(ref["chi"]) <= bnd["chi"])
        if family == "poisson":
            assert weak_d.mean() < 0.01 and weak_c.mean() < 0.01
        else:
            assert not weak_d.any() and not weak_c.any()


def test_hc3_meat_dominates_hc0():
    Z, y, theta, w, o = _small("poisson", True, True, n=200)
    R = RR.factor(RR.information("poisson", Z, theta, w, o))
    h = RR.rows("poisson", Z, y, theta, R, w, o)["leverage"]
    M3 = RR.hc3_meat("poisson", Z, y, theta, h, w, o)
    M0 = GR.gram("poisson", Z, y, theta, w, o)[0]
    assert np.linalg.eigvalsh(M3 - M0).min() >= -1e-12 * np.abs(M0).max()
    assert np.array_equal(RR.hc3_meat("poisson", Z, y, theta, np.zeros(len(y)), w, o), M0)


def test_rows_factor():
    from dlsa_amd.models import rows_factor

    P = 5
    B = np.random.default_rng(2).standard_normal((4, 30, P))
    S = np.einsum("kni,knj->kij", B, B)
    R = rows_factor(S, 4, P)
    for k in range(4):
        assert np.abs(R[k].T @ R[k] @ S[k] - np.eye(P)).max() <= 1e-12
        assert not np.triu(R[k], 1).any()
    assert np.array_equal(rows_factor(S[1], 4, P), R[1])
    S[1, 2, 2] = np.nan
    S[2] = 0.0
    S[3] = -S[3]
    R2 = rows_factor(S, 4, P)
    assert np.array_equal(R2[0], R[0])
    assert all(np.isnan(R2[k]).all() for k in (1, 2, 3))
    v = np.random.default_rng(3).standard_normal((P, 2))  # rank 2 at P = 5
    assert np.isnan(rows_factor(v @ v.T, 1, P)).all()


# ---- Python surface ---------------------------------------------------------------------------

def test_signatures():
    from dlsa_amd import _hip
    from dlsa_amd import distributed as D
    from dlsa_amd import models as M

    ps = inspect.signature(M.glm_rows_batched).parameters
    assert list(ps)[:4] == ["family", "X", "y", "offsets"]
    for name, default in (("thetas", None), ("beta", None), ("info", None), ("outputs", None),
                          ("eta_offset", None), ("exposure", None), ("sample_weight", None),
                          ("fit_intercept", False), ("center", None), ("scale", None),
                          ("rows_per_chunk", 0), ("device", None)):
        assert ps[name].default == default, name
    assert inspect.signature(D.dlsa_fit_sharded).parameters["cov_type"].default is None
    assert "HC3" in D._COV_TYPES and "HC2" not in D._COV_TYPES
    P, I32, I64 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64
    want = [I32, P, P, P, P, P, I32, I32, I32, P, P, P, I64, P, I64, P, P, P, P, P, P]
    assert _hip.SIGNATURES["dlsa_glm_rows_batched"] == (ctypes.c_int, want)
    assert _hip.SIGNATURES["dlsa_glm_rows_batched_chunked"] == (
        ctypes.c_int, want[:15] + [I32] + want[15:])
    lib = ctypes.CDLL(_hip.LIB_PATH)  # exported (the library loads without a GPU)
    assert lib.dlsa_glm_rows_batched and lib.dlsa_glm_rows_batched_chunked


def test_entry_rejects_bad_arguments_before_any_launch():
    """The C entry's argument errors need no GPU: they come before any HIP call."""
    from dlsa_amd import _hip

    lib = _hip.load()
    off = np.array([0, 0], dtype=np.int64)
    offp = off.ctypes.data_as(ctypes.c_void_p)
    buf = np.zeros(200 * 200)
    b = buf.ctypes.data_as(ctypes.c_void_p)

    def call(family=_hip.FAMILY_POISSON, o=None, p=3, ic=1, stride=0, rfac=b, rstride=0, lev=b,
             center=None):
        return lib.dlsa_glm_rows_batched(family, None, None, o, None, offp, 1, p, ic, center,
                                         None, b, stride, rfac, rstride, None, None, None, None,
                                         lev, None)

    assert call() == 0  # an empty job: nothing to write, no launch
    assert call(family=1) == -3  # DLSA_E_UNSUPPORTED: the Gaussian family's code
    assert call(p=192, ic=1) == -3 and "DLSA_MAX_P_FUSED" in _hip.last_error()
    assert call(stride=3) == -1  # DLSA_E_INVALID: neither 0 nor P = 4
    assert call(rstride=4) == -1 and "rfac_part_stride" in _hip.last_error()
    assert call(rstride=16) == 0 and call(stride=4) == 0
    assert call(family=_hip.FAMILY_LOGISTIC, o=b) == -1 and "Poisson" in _hip.last_error()
    assert call(rfac=None) == -1 and "rfac" in _hip.last_error()
    assert call(rfac=None, lev=None) == 0
    assert call(center=b) == -1
    rc = lib.dlsa_glm_rows_batched_chunked(_hip.FAMILY_POISSON, None, None, None, None, offp, 1,
                                           3, 1, None, None, b, 0, b, 0, -1, None, None, None,
                                           None, b, None)
    assert rc == -1


def test_arguments_checked_before_the_gpu(monkeypatch):
    from dlsa_amd import distributed as D
    from dlsa_amd import models as M

    def no_gpu(device=None):
        raise AssertionError("the GPU was touched before the argument check")

    monkeypatch.setattr(M, "_require_gpu", no_gpu)
    n, p = 40, 2
    X, y, off = np.zeros((n, p)), np.zeros(n), np.array([0, 25, n])
    th, be = np.zeros((2, p)), np.zeros(p)
    S = np.stack([np.eye(p)] * 2)
    bad = [
        (dict(), "exactly one"),
        (dict(thetas=th, beta=be), "exactly one"),
        (dict(thetas=th, family="gaussian"), "family"),
        (dict(thetas=th, eta_offset=np.zeros(n)), "poisson"),
        (dict(thetas=th, family="poisson", eta_offset=np.zeros(n), exposure=np.ones(n)),
         "not both"),
        (dict(thetas=th, family="poisson", exposure=np.zeros(n)), "exposure"),
        (dict(thetas=th, sample_weight=-np.ones(n)), "sample_weight"),
        (dict(thetas=th, sample_weight=np.ones(n - 1)), "n entries"),
        (dict(thetas=np.zeros((3, p))), "thetas must be"),
        (dict(beta=np.zeros(p + 1)), "beta must be"),
        (dict(thetas=th, rows_per_chunk=-1), "rows_per_chunk"),
        (dict(thetas=th, center=np.zeros(p)), "center and scale"),
        (dict(thetas=th, outputs=("eta", "hat")), "outputs"),
        (dict(thetas=th, outputs=()), "outputs"),
        (dict(thetas=th, outputs=("leverage",)), "need info"),
        (dict(thetas=th, outputs=("mu", "cooks")), "need info"),
        (dict(thetas=th, info=np.eye(p + 1)), "info must be"),
        (dict(thetas=th, info=np.zeros((3, p, p))), "info must be"),
        (dict(beta=be, info=S[:, :1]), "info must be"),
    ]
    for kw, match in bad:
        kw = dict(kw)
        family = kw.pop("family", "logistic")
        with pytest.raises(ValueError, match=match):
            M.glm_rows_batched(family, X, y, off, **kw)
    # what passes the checks reaches the GPU (and only then fails here)
    for kw in (dict(thetas=th), dict(beta=be, info=S), dict(thetas=th, info=S[0], outputs="cooks")):
        with pytest.raises(AssertionError, match="the GPU was touched"):
            M.glm_rows_batched("logistic", X, y, off, **kw)
    codes = np.zeros((n, 1), np.uint8)
    for kw, match in [
        (dict(cov_type="HC2"), "cov_type"),
        (dict(cov_type="HC3", dispersion="pearson"), "absorbs"),
        (dict(cov_type="HC3", codes=codes, levels=[3]), "dense layout only"),
    ]:
        with pytest.raises(ValueError, match=match):
            D.dlsa_fit_sharded(X, y, off, **kw)


# ---- dlsa_fit_sharded on stubbed passes -------------------------------------------------------

def _spd(P, seed):
    B = np.random.default_rng(seed).standard_normal((4 * P, P))
    return B.T @ B / (4 * P) + np.eye(P)


def _stub_job(monkeypatch, h_of=None):
    """A one-partition logistic job whose fit, reduction, score pass and rows
    pass are numpy stubs; returns (X, y, off, calls)."""
    import torch

    from dlsa_amd import distributed as D
    from dlsa_amd import models as M

    n, P = 60, 3
    rng = np.random.default_rng(7)
    X = rng.standard_normal((n, P)) * 0.5
    theta = np.array([0.4, -0.3, 0.2])
    y = (rng.uniform(size=n) < G._expit(X @ theta)).astype(np.float64)
    A = G.hessian("logistic", X, theta)

    class Fit:
        pass

    fit = Fit()
    fit.P, fit.K = P, 1
    fit.theta = torch.from_numpy(theta[None].copy())
    fit.sig_inv = torch.from_numpy(A[None].copy())
    fit.status = torch.zeros(1, dtype=torch.int32)
    calls = []

    def gram(family, X_, y_, off_, kind="score", thetas=None, sample_weight=None, **kw):
        calls.append(("gram", None if sample_weight is None else
                      np.asarray(sample_weight, np.float64).copy()))
        w = None if sample_weight is None else np.asarray(sample_weight, np.float64)
        Mk = GR.gram(family, np.asarray(X_), np.asarray(y_), np.asarray(thetas)[0], w)[0]
        return {"gram": torch.from_numpy(Mk[None].copy())}

    def gof(family, X_, y_, off_, sample_weight=None, **kw):
        calls.append(("gof", None))
        npos = int((np.asarray(sample_weight) > 0).sum())
        return {"n_pos": torch.tensor([npos], dtype=torch.int64)}

    def rows(family, X_, y_, off_, thetas=None, info=None, outputs=None, **kw):
        calls.append(("rows", tuple(outputs)))
        assert info is fit.sig_inv and thetas is fit.theta
        return {"leverage": torch.from_numpy(np.asarray(h_of(n), np.float64))}

    monkeypatch.setattr(M, "logistic_model_batched", lambda *a, **k: fit)
    monkeypatch.setattr(M, "logistic_model_batched_weighted", lambda *a, **k: fit)
    monkeypatch.setattr(M, "glm_gram_batched", gram)
    monkeypatch.setattr(M, "glm_gof_batched", gof)
    monkeypatch.setattr(M, "glm_rows_batched", rows)
    buf = np.concatenate([A.ravel(), A @ theta, theta, [1.0, float(n)]])
    monkeypatch.setattr(D, "reduce_partitions_device",
                        lambda f, n_rows=False: torch.from_numpy(buf.copy()))
    return X, y, [0, n], calls


def test_cov_types_on_a_stubbed_fit(monkeypatch):
    """HC3 is accepted, HC2 still raises; None and "model" run no new pass and
    give today's keys; HC0 / HC1 take today's calls (no rows pass)."""
    from dlsa_amd import distributed as D

    X, y, off, calls = _stub_job(monkeypatch, h_of=lambda n: np.full(n, 0.05))
    plain = D.dlsa_fit_sharded(X, y, off)
    none = D.dlsa_fit_sharded(X, y, off, cov_type=None)
    model = D.dlsa_fit_sharded(X, y, off, cov_type="model")
    assert calls == []
    assert set(none) == set(plain) and "cov" not in none
    assert set(model) - set(plain) == {"cov", "std_err", "z", "p_value"}
    hc0 = D.dlsa_fit_sharded(X, y, off, cov_type="HC0")
    D.dlsa_fit_sharded(X, y, off, cov_type="HC1")
    assert [c[0] for c in calls] == ["gram", "gram"] and calls[0][1] is None
    del calls[:]
    hc3 = D.dlsa_fit_sharded(X, y, off, cov_type="HC3")
    assert [c[0] for c in calls] == ["rows", "gram"] and calls[0][1] == ("leverage",)
    assert np.array_equal(calls[1][1], np.full(len(y), 1.0 / 0.95))
    assert set(hc3) == set(hc0)
    assert np.array_equal(hc3["wlse"], plain["wlse"])
    assert (hc3["std_err"] > hc0["std_err"]).all()
    assert np.allclose(hc3["cov"], hc0["cov"] / 0.95 ** 2, rtol=1e-12, atol=0)
    with pytest.raises(ValueError, match="cov_type"):
        D.dlsa_fit_sharded(X, y, off, cov_type="HC2")


def test_hc3_with_zero_leverage_is_hc0_to_the_bit(monkeypatch):
    from dlsa_amd import distributed as D

    X, y, off, calls = _stub_job(monkeypatch, h_of=lambda n: np.zeros(n))
    hc0 = D.dlsa_fit_sharded(X, y, off, cov_type="HC0")
    hc3 = D.dlsa_fit_sharded(X, y, off, cov_type="HC3")
    for key in ("cov", "std_err", "meat_sum", "info", "wlse", "z", "p_value"):
        assert np.array_equal(hc3[key], hc0[key]), key
    # weights: omega / (1 - h) = omega, rows with omega = 0 stay out
    w = np.ones(len(y))
    w[::7] = 0.0
    del calls[:]
    hc0 = D.dlsa_fit_sharded(X, y, off, cov_type="HC0", sample_weight=w)
    hc3 = D.dlsa_fit_sharded(X, y, off, cov_type="HC3", sample_weight=w)
    assert np.array_equal(hc3["cov"], hc0["cov"])
    assert np.array_equal([c for c in calls if c[0] == "gram"][-1][1], w)


@pytest.mark.parametrize("bad", [1.0, 1.5, np.nan, np.inf])
def test_hc3_raises_where_it_is_undefined(monkeypatch, bad):
    from dlsa_amd import distributed as D

    def h_of(n):
        h = np.full(n, 0.1)
        h[11] = bad
        return h

    X, y, off, _ = _stub_job(monkeypatch, h_of=h_of)
    with pytest.raises(ValueError, match="partition 0"):
        D.dlsa_fit_sharded(X, y, off, cov_type="HC3")
    w = np.ones(len(y))
    w[11] = 0.0  # the row carries no weight: HC3 is defined without it
    out = D.dlsa_fit_sharded(X, y, off, cov_type="HC3", sample_weight=w)
    assert np.isfinite(out["cov"]).all()
