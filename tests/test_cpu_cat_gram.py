"""No GPU: the score outer-product pass on the categorical-code layout
(``glm_gram_batched_categorical``, ``gram_sharded(codes=)``,
``sandwich_sharded``) -- the argument checks before the GPU is touched, the
sandwich tail on stubbed passes for both layouts, the C entry's errors that
need no launch, and the condition on the inputs of tests/test_gpu_cat_gram.py:
the a-priori fixed-point bound of every case it runs (tests/_cat_gram_ref.py)
is at most 2.5e-11, a quarter of its 1e-10 tolerance.
"""

import ctypes
import inspect

import numpy as np
import pytest

import _cat_gram_ref as CR
import _glm_ref as G
import _gram_ref as GR


def test_signatures():
    from dlsa_amd import _hip
    from dlsa_amd import distributed as D
    from dlsa_amd import models as M

    ps = inspect.signature(M.glm_gram_batched_categorical).parameters
    assert list(ps)[:6] == ["family", "Xn", "codes", "y", "offsets", "levels"]
    dense = inspect.signature(M.glm_gram_batched).parameters
    for name in list(dense)[4:]:
        assert ps[name].default == dense[name].default, name
    ps = inspect.signature(D.gram_sharded).parameters
    assert ps["codes"].default is None and ps["levels"].default is None
    ps = inspect.signature(D.sandwich_sharded).parameters
    assert list(ps)[:4] == ["fit", "X", "y", "offsets"]
    for name, default in (("cov_type", "HC0"), ("codes", None), ("levels", None),
                          ("family", "logistic"), ("eta_offset", None), ("exposure", None),
                          ("sample_weight", None), ("fit_intercept", False), ("center", None),
                          ("scale", None), ("lars_type", "lasso"), ("group", None)):
        assert ps[name].default == default, name
    P, I32, I64 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64
    want = [I32, I32, P, P, P, P, P, P, I32, I32, I32, P, I32, P, P, P, I64, I32, P, P, P, P, P]
    assert _hip.SIGNATURES["dlsa_glm_gram_categorical"] == (ctypes.c_int, want)
    lib = ctypes.CDLL(_hip.LIB_PATH)  # exported (the library loads without a GPU)
    assert lib.dlsa_glm_gram_categorical


def test_entry_rejects_bad_arguments_before_any_launch():
    """The C entry's argument errors need no GPU: they come before any HIP call."""
    from dlsa_amd import _hip

    lib = _hip.load()
    off = np.array([0, 0], dtype=np.int64)
    offp = off.ctypes.data_as(ctypes.c_void_p)
    buf = np.zeros(200 * 200)
    b = buf.ctypes.data_as(ctypes.c_void_p)

    def call(family=_hip.FAMILY_POISSON, kind=0, o=None, q=3, levels=(4, 3), ic=1, stride=0,
             rpc=0):
        lv = np.asarray(levels, dtype=np.int32)
        return lib.dlsa_glm_gram_categorical(
            family, kind, None, None, None, o, None, offp, 1, q, len(lv),
            lv.ctypes.data_as(ctypes.c_void_p), ic, None, None, b, stride, rpc, b, b, None, None,
            None)

    assert call(family=1) == -3  # DLSA_E_UNSUPPORTED: the Gaussian family's code
    assert call(q=16) == -3  # intercept + q > 16
    assert call(levels=(100, 100)) == -3  # P = 1 + 3 + 198 > 192
    assert call(levels=(300,)) == -1  # a level count no uint8 code reaches
    assert call(stride=3) == -1  # DLSA_E_INVALID: neither 0 nor P = 9
    assert call(family=_hip.FAMILY_LOGISTIC, o=b) == -1 and "Poisson" in _hip.last_error()
    assert call(kind=2) == -1 and call(rpc=-1) == -1


def test_arguments_checked_before_the_gpu(monkeypatch):
    from dlsa_amd import distributed as D
    from dlsa_amd import models as M

    def no_gpu(device=None):
        raise AssertionError("the GPU was touched before the argument check")

    monkeypatch.setattr(M, "_require_gpu", no_gpu)
    n, q, levels = 40, 2, [3, 2]
    P = q + 3
    Xn, y, off = np.zeros((n, q)), np.zeros(n), np.array([0, 25, n])
    codes = np.zeros((n, 2), np.uint8)
    th, be = np.zeros((2, P)), np.zeros(P)
    bad = [
        (dict(thetas=th, kind="meat"), "kind"),
        (dict(), "exactly one"),
        (dict(thetas=th, beta=be), "exactly one"),
        (dict(thetas=th, family="gaussian"), "family"),
        (dict(thetas=th, eta_offset=np.zeros(n)), "poisson"),
        (dict(thetas=th, family="poisson", eta_offset=np.zeros(n), exposure=np.ones(n)),
         "not both"),
        (dict(thetas=th, family="poisson", exposure=np.zeros(n)), "exposure"),
        (dict(thetas=th, sample_weight=-np.ones(n)), "sample_weight"),
        (dict(thetas=th, sample_weight=np.ones(n - 1)), "n entries"),
        (dict(thetas=np.zeros((3, P))), "thetas must be"),
        (dict(thetas=np.zeros((2, q))), "thetas must be"),  # the dense design's P
        (dict(beta=np.zeros(P + 1)), "beta must be"),
        (dict(thetas=th, rows_per_chunk=-1), "rows_per_chunk"),
        (dict(thetas=th, center=np.zeros(q)), "center and scale"),
        (dict(thetas=th, center=np.zeros(P), scale=np.ones(P)), "center and scale"),
    ]
    for kw, match in bad:
        kw = dict(kw)
        family = kw.pop("family", "logistic")
        with pytest.raises(ValueError, match=match):
            M.glm_gram_batched_categorical(family, Xn, codes, y, off, levels, **kw)
        with pytest.raises(ValueError, match=match):
            D.gram_sharded(Xn, y, off, family=family, codes=codes, levels=levels, **kw)
    with pytest.raises(ValueError, match="levels must have F"):
        M.glm_gram_batched_categorical("logistic", Xn, codes, y, off, [3], thetas=th)
    with pytest.raises(ValueError, match="codes must be"):
        M.glm_gram_batched_categorical("logistic", Xn, codes[:-1], y, off, levels, thetas=th)
    with pytest.raises(ValueError, match="offsets"):
        M.glm_gram_batched_categorical("logistic", Xn, codes, y, [0, 25, n + 1], levels, thetas=th)
    # a good call gets as far as the GPU
    with pytest.raises(AssertionError, match="the GPU was touched"):
        M.glm_gram_batched_categorical("logistic", Xn, codes, y, off, levels, thetas=th)
    with pytest.raises(AssertionError, match="the GPU was touched"):
        D.gram_sharded(Xn, y, off, codes=codes, levels=levels, beta=be)
    # sandwich_sharded: its own checks come before the reduction and the passes
    for kw, match in [(dict(cov_type="HC2"), "cov_type"), (dict(cov_type=None), "cov_type"),
                      (dict(cov_type="model"), "cov_type"),
                      (dict(cov_type="HC3", codes=codes, levels=levels), "dense layout only"),
                      (dict(family="gaussian"), "family"),
                      (dict(eta_offset=np.zeros(n)), "poisson")]:
        with pytest.raises(ValueError, match=match):
            D.sandwich_sharded(None, Xn, y, off, **kw)


# ---- sandwich_sharded on stubbed passes -------------------------------------------------------

def _stub_job(monkeypatch, layout):
    """A logistic job of three partitions (the middle one SINGULAR: the combine
    does not count it) whose reduction, score pass and goodness-of-fit pass are
    numpy stubs; returns (fit, X, y, off, kw, Z, thetas, calls).  layout
    "codes": X holds one numeric column, beside one factor of three levels."""
    import torch

    import oracle as O
    from dlsa_amd import distributed as D
    from dlsa_amd import models as M

    sizes = (60, 40, 50)
    off = np.concatenate([[0], np.cumsum(sizes)])
    n = int(off[-1])
    rng = np.random.default_rng(7)
    if layout == "codes":
        X = rng.standard_normal((n, 1)) * 0.5
        codes = rng.integers(0, 3, (n, 1)).astype(np.uint8)
        Z = O.expand_codes(X, codes, [3])
        kw = dict(codes=codes, levels=[3])
    else:
        X = rng.standard_normal((n, 3)) * 0.5
        Z, kw = X, {}
    P = 3
    thetas = np.array([[0.4, -0.3, 0.2], [9.0, 9.0, 9.0], [0.3, -0.2, 0.1]])
    y = (rng.uniform(size=n) < G._expit(Z @ thetas[0])).astype(np.float64)
    status = np.array([0, 2, 1], dtype=np.int32)
    ok = status <= 1
    A = [G.hessian("logistic", Z[a:b], thetas[k]) for k, (a, b) in enumerate(zip(off, off[1:]))]

    class Fit:
        pass

    fit = Fit()
    fit.P, fit.K = P, 3
    fit.theta = torch.from_numpy(thetas.copy())
    fit.status = torch.from_numpy(status)
    calls = []

    def gram_of(Zfull, family, y_, off_, kind, thetas, sample_weight):
        Mk = GR.gram_partitions(family, Zfull, np.asarray(y_), np.asarray(off_),
                                thetas=np.asarray(thetas), w=sample_weight, kind=kind)[0]
        return {"gram": torch.from_numpy(Mk.copy())}

    def gram(family, X_, y_, off_, kind="score", thetas=None, sample_weight=None, **k):
        calls.append("gram")
        return gram_of(np.asarray(X_), family, y_, off_, kind, thetas, sample_weight)

    def gram_cat(family, X_, codes_, y_, off_, levels_, kind="score", thetas=None,
                 sample_weight=None, **k):
        calls.append("gram_cat")
        return gram_of(O.expand_codes(np.asarray(X_), codes_, levels_), family, y_, off_, kind,
                       thetas, sample_weight)

    def npos_of(off_, w):
        return {"n_pos": torch.tensor([int((np.asarray(w)[a:b] > 0).sum())
                                       for a, b in zip(off_, off_[1:])], dtype=torch.int64)}

    def gof(family, X_, y_, off_, sample_weight=None, **k):
        calls.append("gof")
        return npos_of(off_, sample_weight)

    def gof_cat(family, X_, codes_, y_, off_, levels_, sample_weight=None, **k):
        calls.append("gof_cat")
        return npos_of(off_, sample_weight)

    monkeypatch.setattr(M, "glm_gram_batched", gram)
    monkeypatch.setattr(M, "glm_gram_batched_categorical", gram_cat)
    monkeypatch.setattr(M, "glm_gof_batched", gof)
    monkeypatch.setattr(M, "glm_gof_batched_categorical", gof_cat)
    S = sum(A[k] for k in range(3) if ok[k])
    v = sum(A[k] @ thetas[k] for k in range(3) if ok[k])
    buf = np.concatenate([S.ravel(), v, thetas[ok].sum(0), [float(ok.sum()), float(n)]])
    monkeypatch.setattr(D, "reduce_partitions_device",
                        lambda f, n_rows=False: torch.from_numpy(buf.copy()))
    return fit, X, y, off, kw, Z, thetas, calls, S, ok


@pytest.mark.parametrize("layout", ["dense", "codes"])
def test_sandwich_sharded_on_stubbed_passes(monkeypatch, layout):
    """It sums the meat of the counted partitions only, HC1 is HC0 times n+ /
    (n+ - K_ok P) with n+ from the layout's own goodness-of-fit pass, HC3 on
    codes and a bad cov_type raise, and the keys are dlsa_fit_sharded's."""
    from dlsa_amd import distributed as D

    fit, X, y, off, kw, Z, thetas, calls, S, ok = _stub_job(monkeypatch, layout)
    P = 3
    sfx = "_cat" if layout == "codes" else ""
    Mk = GR.gram_partitions("logistic", Z, y, off, thetas=thetas)[0]
    Mref = Mk[0] + Mk[2]  # partition 1 (SINGULAR) is not counted
    hc0 = D.sandwich_sharded(fit, X, y, off, **kw)
    assert calls == ["gram" + sfx]
    assert set(hc0) == {"wlse", "oneshot", "beta_byAIC", "beta_byBIC", "dbic_support", "path",
                        "Sig_inv_sum", "info", "meat_sum", "cov", "std_err", "z", "p_value"}
    assert np.abs(hc0["meat_sum"] - Mref).max() <= 1e-13 * np.abs(Mref).max()
    cov_ref, info_ref = GR.sandwich(S, Mref)
    assert np.abs(hc0["cov"] - cov_ref).max() <= 1e-10 * np.abs(cov_ref).max()
    assert np.abs(hc0["info"] - info_ref).max() <= 1e-10 * np.abs(info_ref).max()
    # HC1 without weights: n+ is the counted partitions' rows, no more pass
    del calls[:]
    hc1 = D.sandwich_sharded(fit, X, y, off, cov_type="HC1", **kw)
    assert calls == ["gram" + sfx]
    npos = (off[1] - off[0]) + (off[3] - off[2])
    assert np.allclose(hc1["cov"], hc0["cov"] * npos / (npos - 2 * P), rtol=1e-12, atol=0)
    # ... with weights: the layout's goodness-of-fit pass counts omega > 0
    w = np.ones(len(y))
    w[::7] = 0.0
    del calls[:]
    h0w = D.sandwich_sharded(fit, X, y, off, cov_type="HC0", sample_weight=w, **kw)
    h1w = D.sandwich_sharded(fit, X, y, off, cov_type="HC1", sample_weight=w, **kw)
    assert calls == ["gram" + sfx, "gof" + sfx, "gram" + sfx, "gof" + sfx]
    npos = int((w[off[0]:off[1]] > 0).sum() + (w[off[2]:off[3]] > 0).sum())
    assert np.allclose(h1w["cov"], h0w["cov"] * npos / (npos - 2 * P), rtol=1e-12, atol=0)
    with pytest.raises(ValueError, match="cov_type"):
        D.sandwich_sharded(fit, X, y, off, cov_type="HC2", **kw)
    if layout == "codes":
        with pytest.raises(ValueError, match="HC3"):
            D.sandwich_sharded(fit, X, y, off, cov_type="HC3", **kw)
    with pytest.raises(ValueError, match="degrees of freedom"):
        few = np.zeros(len(y))
        few[:3] = 1.0
        D.sandwich_sharded(fit, X, y, off, cov_type="HC1", sample_weight=few, **kw)


# ---- the condition on the GPU cases' inputs ---------------------------------------------------

@pytest.mark.parametrize("shape", CR.SHAPES, ids=CR.SHAPE_IDS)
def test_a_priori_bound_of_the_gpu_cases(shape):
    """n_k R 2^-60 2 B per entry class, relative to the block's largest entry
    (the score: to max |Z|^T |s|), is at most 2.5e-11 for every family, mask,
    kind and coefficient choice tests/test_gpu_cat_gram.py runs."""
    d = CR.case(shape)
    worst = 0.0
    for family, mask in CR.FAMILY_MASKS:
        o, w = CR.extras(d, mask)
        for kind in CR.KINDS:
            for coef in (d["thetas"], d["beta"]):
                bg, bs = CR.bound(family, d["Z"], d[family], d["off"], coef, d["q"], d["fi"],
                                  d["rpc"], w=w, o=o, kind=kind)
                worst = max(worst, bg.max(), bs.max())
                assert bg.max() <= CR.BOUND_MAX and bs.max() <= CR.BOUND_MAX, \
                    (family, mask, kind, bg, bs)
    print(f"{shape[:2]}: worst a-priori bound {worst:.2e}")


def test_max_chunk_rows():
    assert CR.max_chunk_rows([0, 3000, 3000, 9000, 12000], 0) == 1024
    assert CR.max_chunk_rows([0, 3001], 1500) == 1024  # 3 chunks of 1001 rows
    assert CR.max_chunk_rows([0, 3001, 7001], 2000) == 2000
    assert CR.max_chunk_rows([0, 10 ** 6], 0) == 1954  # 512 chunks
