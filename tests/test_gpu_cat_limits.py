"""GPU: every entry point of the categorical-code layout at the limits
include/dlsa_hip.h documents -- F = 16 factors, P = 192, intercept + q = 16
with and without an intercept, codes up to 192 -- on the ten shapes of
tests/_cat_limits.py (A-J), whose layouts need up to four passes of
``cat_layout``'s shrink loop, fill the 120-entry pair table, mix 16-fold
replicated with unreplicated histograms, and in J leave 48 bytes of the LDS.
tests/test_cpu_cat_limits.py checks in numpy that the shapes reach what that
module's table says and that the data can carry the tolerances.

Yardstick throughout: the fp64 numpy reference on ``oracle.expand_codes``
(tests/_glm_ref.py, _gof_ref.py, _gram_ref.py).  Tolerances are the neighbouring
modules', imported: the fits at tests/test_gpu_pois_cat.py's REL / REL_S /
REL_LL with tol = TOL through its ``_compare``, the log-likelihood passes at
tests/test_gpu_eval.py's TOL, goodness of fit at tests/test_gpu_gof.py's REL,
the Gram pass at tests/_cat_gram_ref.py's TOL and within its a-priori bound.
Every comparison prints its figures per partition before it asserts.

Measured on an MI355X, the largest over partitions, families and masks (the
fits against 1e-8 / 1e-10 / 1e-8 / 1e-9, the log-likelihood pass against 1e-10,
goodness of fit against 1e-12, gram and score against 1e-10 and the a-priori
bound; "-": the entry is not run on that shape):

    id  theta    Sig_inv  Sig_inv theta  loglik   ll pass  gof      gram     score
    A   7.6e-15  1.7e-12  6.4e-13        2.8e-16  3.4e-16  4.3e-16  3.3e-15  8.5e-16
    B   2.6e-15  2.4e-12  7.1e-13        3.7e-16  4.3e-16  3.5e-16     -        -
    C   1.6e-14  6.3e-14  1.7e-14        3.6e-16  2.7e-16     -     3.7e-15  9.1e-16
    D   1.6e-14  1.7e-12  2.3e-13        1.9e-16  3.0e-16  3.9e-16  6.9e-15  1.0e-15
    E   6.4e-15  5.1e-15  7.8e-16        4.0e-16  3.7e-16     -        -        -
    F   9.2e-15  5.7e-15  3.3e-15        2.8e-16  3.8e-16     -     1.9e-15  2.5e-15
    G   1.3e-14  1.1e-12  2.9e-14        2.5e-16  3.0e-16  3.5e-16  2.5e-15  1.1e-15
    H   1.4e-14  1.7e-12  1.7e-12        2.6e-16  3.5e-16  3.4e-16     -        -
    I   6.8e-14  2.9e-13  3.8e-14        3.2e-16  3.3e-16     -     1.2e-15  1.8e-15
    J   2.7e-15  2.6e-15  1.1e-15        2.8e-16  3.3e-16  3.3e-16  2.2e-14  1.8e-15

Shape A in chunks of 1024 rows gives A's row; the dense weighted fit of the
expanded design agrees with the categorical fit of A and G within 1.3e-14
(theta) and 1.1e-14 (Sig_inv per entry).  The figures near 1e-12 are the
rounding of the histograms' fixed-point grids (the Poisson family's are sized
from a bound on eta).
"""

import ctypes

import numpy as np
import pytest

import _cat_gram_ref as CR
import _cat_limits as L
import _glm_ref as G
import _gof_ref as GR
import _gram_ref as R
import _poison as PZ
import test_gpu_cat_weighted as CW
import test_gpu_eval as EV
import test_gpu_gof as GF
import test_gpu_pois_cat as PC

pytestmark = pytest.mark.gpu

FM = CR.FAMILY_MASKS
FM_IDS = [f"{f}-{m}" for f, m in FM]
OK_STATUS = [0, PZ.STATUS_EMPTY, 0]
E_INVALID, E_UNSUPPORTED = -1, -3  # DLSA_E_INVALID, DLSA_E_UNSUPPORTED


@pytest.fixture(scope="module")
def M():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a visible MI355X"
    from dlsa_amd import models
    return models


def _kw(d, **over):
    return dict(dict(fit_intercept=d["fi"], center=d["center"], scale=d["scale"],
                     rows_per_chunk=d["rpc"]), **over)


def _fit(M, d, family, mask, **over):
    o, w = L.extras(d, mask)
    args = (d["Xn"], d["codes"], d[family], d["off"], d["levels"])
    kw = _kw(d, tol=PC.TOL, **over)
    if family == "poisson":
        return M.poisson_model_batched_categorical(*args, sample_weight=w, eta_offset=o, **kw)
    if w is None:
        return M.logistic_model_batched_categorical(*args, **kw)
    return M.logistic_model_batched_categorical_weighted(*args, sample_weight=w, **kw)


def _fit_against_numpy(M, sid, family, mask, tag, **over):
    d = L.case(sid)
    got = PC._host(_fit(M, d, family, mask, **over))
    assert got["status"].tolist() == OK_STATUS, (tag, got["status"])  # (none "unsupported")
    assert got["theta"].shape == (3, d["P"])
    for f in ("theta", "sig_inv", "sig_inv_theta", "loglik", "iters"):
        assert not got[f][L.EMPTY_AT].any(), f
    ref = dict(L.ref_fit(sid, family, mask))
    ref["status"] = got["status"]
    PC._compare(got, ref, tag)


# ---- 1. the fits ---------------------------------------------------------------------------------

@pytest.mark.parametrize("family,mask", FM, ids=FM_IDS)
@pytest.mark.parametrize("sid", L.IDS)
def test_fit_vs_numpy(M, sid, family, mask):
    _fit_against_numpy(M, sid, family, mask, f"fit {sid} {family}-{mask}")


@pytest.mark.parametrize("family", ["logistic", "poisson"])
@pytest.mark.parametrize("sid", ["A", "G"])
def test_fit_vs_dense_weighted(M, sid, family):
    """The library's dense weighted fit of the expanded design (P = 192, the
    fused path's limit) against the categorical fit."""
    import torch

    d = L.case(sid)
    mask = "both" if family == "poisson" else "wgt"
    o, w = L.extras(d, mask)
    got = PC._host(_fit(M, d, family, mask))
    X = M.expand_categorical(torch.from_numpy(d["Xn"]).cuda(), torch.from_numpy(d["codes"]).cuda(),
                             d["levels"])
    assert X.shape[1] + 1 == d["P"] == 192
    kw = dict(sample_weight=w, fit_intercept=d["fi"], hessian="fp64", tol=PC.TOL)
    if family == "poisson":
        want = M.poisson_model_batched_weighted(X, d[family], d["off"], eta_offset=o, **kw)
    else:
        want = M.logistic_model_batched_weighted(X, d[family], d["off"], **kw)
    want = PC._host(want)
    assert want["status"].tolist() == OK_STATUS
    PC._compare(got, want, f"dense {sid} {family}-{mask}", iters_pm1=True)


# ---- 2. the log-likelihood passes ----------------------------------------------------------------

def _np_loglik(d, family, mask, betas):
    o, w = L.extras(d, mask)
    off, y, Z = d["off"], d[family], d["Z"]
    return np.array([[G.loglik(family, Z[a:b], y[a:b], bt, None if w is None else w[a:b],
                               None if o is None else o[a:b]) if b > a else 0.0 for bt in betas]
                     for a, b in zip(off[:-1], off[1:])])


@pytest.mark.parametrize("family,mask", FM, ids=FM_IDS)
@pytest.mark.parametrize("sid", L.IDS)
def test_loglik_vs_numpy(M, sid, family, mask):
    """B = 1 and 4 candidates, and on A and B the most of one pass; per
    partition and summed, tests/test_gpu_eval.py::_check's statement.  (The
    wrappers of these passes take ``betas`` only.)"""
    d = L.case(sid)
    o, w = L.extras(d, mask)
    args = (d["Xn"], d["codes"], d[family], d["off"], d["levels"])
    assert M.MAX_LOGLIK_CANDIDATES <= L.N_BETAS
    for B in (1, 4) + ((M.MAX_LOGLIK_CANDIDATES,) if sid in "AB" else ()):
        betas = d["betas"][:B]
        ref = _np_loglik(d, family, mask, betas)
        kw = _kw(d, return_sum=True, sample_weight=w)
        if family == "poisson":
            ll, tot = M.poisson_loglik_batched_categorical(*args, betas, eta_offset=o, **kw)
        else:
            ll, tot = M.logistic_loglik_batched_categorical(*args, betas, **kw)
        assert not ll[L.EMPTY_AT].cpu().numpy().view(np.uint64).any()
        print(f"loglik {sid} {family}-{mask} B={B}")
        EV._check(ll, tot, ref)


# ---- 3. goodness of fit --------------------------------------------------------------------------

@pytest.mark.parametrize("family,mask", FM, ids=FM_IDS)
@pytest.mark.parametrize("sid", ["A", "B", "D", "G", "H", "J"])
def test_gof_vs_numpy(M, sid, family, mask):
    """One candidate, the most of one pass, and each partition at its own
    theta."""
    d = L.case(sid)
    o, w = L.extras(d, mask)
    y, off = d[family], d["off"]
    args = (family, d["Xn"], d["codes"], y, off, d["levels"])
    kw = _kw(d, eta_offset=o, sample_weight=w)
    assert M.MAX_GOF_CANDIDATES <= L.N_BETAS
    for B in (1, M.MAX_GOF_CANDIDATES):
        betas = d["betas"][:B]
        want = GR.gof_partitions(family, d["Z"], y, off, betas=betas, w=w, o=o)
        got = GF._host(M.glm_gof_batched_categorical(*args, betas=betas, return_sum=True, **kw))
        what = f"gof {sid} {family}-{mask} B={B}"
        GF._check(got, want, what)
        GF._check_sums(got, what)
    want = GR.gof_partitions(family, d["Z"], y, off, thetas=d["thetas"], w=w, o=o)
    got = GF._host(M.glm_gof_batched_categorical(*args, thetas=d["thetas"], **kw))
    GF._check(got, want, f"gof {sid} {family}-{mask} own thetas")


# ---- 4. the Gram pass ----------------------------------------------------------------------------

def _gram_call(M, d, family, mask, **kw):
    o, w = L.extras(d, mask)
    return M.glm_gram_batched_categorical(family, d["Xn"], d["codes"], d[family], d["off"],
                                          d["levels"], **_kw(d, eta_offset=o, sample_weight=w,
                                                             **kw))


def _check_gram(got, want, bounds, what):
    """Per partition: gram within CR.TOL of the block's largest entry and score
    within CR.TOL of max |Z|^T |s|, and both within the a-priori bound of the
    fixed-point histograms (+ 1e-13 for the fp64 sums on either side, as
    tests/test_gpu_cat_gram.py::test_heavy_row allows); exact symmetry; the
    empty partition all-zero bits."""
    Gw, sw, scale = want
    bg, bs = bounds
    for k in range(Gw.shape[0]):
        a, b = got["gram"][k], Gw[k]
        assert np.array_equal(a, a.T), (what, k, "gram is not exactly symmetric")
        if k == L.EMPTY_AT:
            assert not b.any()
            assert not a.view(np.uint64).any() and not got["score"][k].view(np.uint64).any()
            continue
        eg = float(np.abs(a - b).max() / np.abs(b).max())
        es = float(np.abs(got["score"][k] - sw[k]).max() / scale[k])
        print(f"{what} k={k}: gram {eg:.3e} (bound {bg[k]:.3e}) score {es:.3e} "
              f"(bound {bs[k]:.3e})")
        assert eg <= CR.TOL and es <= CR.TOL, (what, k, eg, es)
        assert eg <= bg[k] + 1e-13 and es <= bs[k] + 1e-13, (what, k, eg, bg[k], es, bs[k])


@pytest.mark.parametrize("family,mask", FM, ids=FM_IDS)
@pytest.mark.parametrize("sid", ["A", "C", "D", "F", "G", "I", "J"])
def test_gram_vs_numpy(M, sid, family, mask):
    """Both kinds, at own thetas and at the shared beta."""
    d = L.case(sid)
    o, w = L.extras(d, mask)
    for kind in CR.KINDS:
        for own in (True, False):
            sel = dict(thetas=d["thetas"]) if own else dict(beta=d["beta"])
            got = GF._host(_gram_call(M, d, family, mask, kind=kind, return_sum=True, **sel))
            want = R.gram_partitions(family, d["Z"], d[family], d["off"], w=w, o=o, kind=kind,
                                     **sel)
            bounds = CR.bound(family, d["Z"], d[family], d["off"],
                              d["thetas"] if own else d["beta"], d["q"], d["fi"], d["rpc"], w=w,
                              o=o, kind=kind)
            assert max(bounds[0].max(), bounds[1].max()) <= CR.BOUND_MAX
            what = f"gram {sid} {family}-{mask} {kind} own={int(own)}"
            _check_gram(got, want, bounds, what)
            for name in ("gram", "score"):
                acc = np.zeros(got[name].shape[1:])
                for blk in got[name]:  # k ascending
                    acc = acc + blk
                assert PZ.bits_equal(got[name + "_sum"], acc), (what, name + "_sum")


# ---- 5. bit identity -----------------------------------------------------------------------------

@pytest.mark.parametrize("sid", ["A", "D"])
def test_two_fits_give_the_same_bits(M, sid):
    import torch

    d = L.case(sid)
    for family, mask in (("logistic", "wgt"), ("poisson", "both")):
        a, b = _fit(M, d, family, mask), _fit(M, d, family, mask)
        assert a.status.cpu().tolist() == OK_STATUS
        for f in PC.FIELDS:
            assert torch.equal(getattr(a, f), getattr(b, f)), (sid, family, f)


def test_two_gram_passes_give_the_same_bits(M):
    import torch

    d = L.case("A")
    for family, mask in (("logistic", "wgt"), ("poisson", "both")):
        for kind in CR.KINDS:
            g = [_gram_call(M, d, family, mask, kind=kind, thetas=d["thetas"], return_sum=True)
                 for _ in range(2)]
            assert all(torch.equal(g[0][k], g[1][k]) for k in g[0]), (family, kind)


# ---- 6. many workgroups with the 149 KB layout ---------------------------------------------------

@pytest.mark.parametrize("family,mask", FM, ids=FM_IDS)
def test_shape_A_in_chunks_of_1024_rows(M, family, mask):
    """12-16 workgroups per partition, each with the four-times-shrunk layout:
    the tolerances of test_fit_vs_numpy (sums may differ in their last bits from
    the automatic plan's, so no bit equality)."""
    _fit_against_numpy(M, "A", family, mask, f"fit A rpc=1024 {family}-{mask}",
                       rows_per_chunk=1024)


# ---- 7. edges ------------------------------------------------------------------------------------

def test_shape_G_top_level_missing_in_one_partition(M):
    """Level 180 without a row in the last partition: MISSING_LEVEL and zero
    outputs there, the other partition's bits untouched."""
    d = L.case("G")
    off = d["off"]
    codes = d["codes"].copy()
    last = codes[off[2]:off[3], 0]
    assert (last == 180).sum() >= 30
    last[last == 180] = 179
    for family, mask in (("logistic", "none"), ("logistic", "wgt"), ("poisson", "both")):
        clean = PC._host(_fit(M, d, family, mask))
        got = PC._host(_fit(M, dict(d, codes=codes), family, mask))
        assert clean["status"].tolist() == OK_STATUS
        assert got["status"].tolist() == [0, PZ.STATUS_EMPTY, PC.STATUS_MISSING_LEVEL]
        for f in ("theta", "sig_inv", "sig_inv_theta", "loglik", "iters"):
            assert not got[f][2].any(), (family, f)
            assert PZ.bits_equal(got[f][0], clean[f][0]), (family, f)


def test_shape_G_code_one_past_the_last_is_refused(M):
    """Code 181 with levels = 181 -- the boundary, not 255: DLSA_E_INVALID
    ("level codes") from every entry point, through the C ABI for the fits."""
    from dlsa_amd import _hip

    d = L.case("G")
    off = d["off"]
    codes = d["codes"].copy()
    codes[int(off[2]) + 4321, 0] = 181
    bad = dict(d, codes=codes)
    shape = d["shape"]
    rc, _ = PC._abi_fit(shape, d["Xn"], codes, d["poisson"], d["o"], d["w"], off)
    assert rc == E_INVALID and "level codes" in _hip.last_error()
    rc, _ = CW._abi_fit(shape, d["Xn"], codes, d["logistic"], d["w"], off)
    assert rc == E_INVALID and "level codes" in _hip.last_error()
    rc, _ = CW._abi_fit(shape, d["Xn"], codes, d["logistic"], None, off,
                        entry="dlsa_logistic_fit_categorical")
    assert rc == E_INVALID and "level codes" in _hip.last_error()
    args = (d["Xn"], codes, d["poisson"], off, d["levels"])
    calls = [
        lambda: _fit(M, bad, "logistic", "none"),
        lambda: _fit(M, bad, "logistic", "wgt"),
        lambda: _fit(M, bad, "poisson", "both"),
        lambda: M.logistic_loglik_batched_categorical(d["Xn"], codes, d["logistic"], off,
                                                      d["levels"], d["betas"][:2], **_kw(d)),
        lambda: M.logistic_loglik_batched_categorical(d["Xn"], codes, d["logistic"], off,
                                                      d["levels"], d["betas"][:2],
                                                      sample_weight=d["w"], **_kw(d)),
        lambda: M.poisson_loglik_batched_categorical(*args, d["betas"][:2], eta_offset=d["o"],
                                                     sample_weight=d["w"], **_kw(d)),
        lambda: M.glm_gof_batched_categorical("poisson", *args, betas=d["betas"][:2], **_kw(d)),
        lambda: M.glm_gof_batched_categorical("logistic", d["Xn"], codes, d["logistic"], off,
                                              d["levels"], betas=d["betas"][:2], **_kw(d)),
        lambda: _gram_call(M, bad, "poisson", "both", kind="score", thetas=d["thetas"]),
        lambda: _gram_call(M, bad, "logistic", "wgt", kind="information", beta=d["beta"]),
    ]
    for call in calls:
        with pytest.raises(_hip.DlsaHipError, match="level codes"):
            call()
    # the clean codes are accepted afterwards
    assert PC._host(_fit(M, d, "logistic", "none"))["status"].tolist() == OK_STATUS


def _untouched(outs, fill=7):
    for f, v in outs.items():
        assert (np.ascontiguousarray(v).view(np.uint8) == fill).all(), f


def test_shapes_past_the_limits_are_refused_before_any_launch(M):
    """F = 17 and levels = 257: DLSA_E_INVALID; P = 193 (shape A with one factor
    of 13 levels): DLSA_E_UNSUPPORTED; the pre-filled outputs keep their bytes."""
    import torch

    from dlsa_amd import _hip

    n = 64
    off = np.array([0, n], dtype=np.int64)
    y, o, w = np.ones(n), np.zeros(n), np.ones(n)
    cases = [((1, (2,) * 17, True, False, 0), E_INVALID, "F <= 16"),
             ((1, (257,), True, False, 0), E_INVALID, "1..256"),
             ((15, (12,) * 15 + (13,), True, False, 0), E_UNSUPPORTED, "P = 193")]
    for shape, want, text in cases:
        q, levels = shape[0], shape[1]
        Xn, codes = np.zeros((n, q)), np.zeros((n, len(levels)), np.uint8)
        rc, outs = PC._abi_fit(shape, Xn, codes, y, o, w, off)
        assert rc == want and text in _hip.last_error(), (shape[:2], rc, _hip.last_error())
        _untouched(outs)
        rc, outs = CW._abi_fit(shape, Xn, codes, y, w, off)
        assert rc == want and text in _hip.last_error(), (shape[:2], rc, _hip.last_error())
        _untouched(outs)
        rc, outs = CW._abi_fit(shape, Xn, codes, y, None, off,
                               entry="dlsa_logistic_fit_categorical")
        assert rc == want and text in _hip.last_error(), (shape[:2], rc, _hip.last_error())
        _untouched(outs)
        # the Gram entry: the same checks of the shape
        P = L.n_params(shape)
        lv = np.asarray(levels, dtype=np.int32)
        dev = torch.device("cuda")
        t = [torch.from_numpy(a).to(dev) for a in (Xn, codes, y)]
        beta = torch.zeros(P, dtype=torch.float64, device=dev)
        out = torch.full((8 * (P * P + P),), 7, dtype=torch.uint8, device=dev)
        gram = out.view(torch.float64)
        rc = _hip.load().dlsa_glm_gram_categorical(
            _hip.FAMILY_LOGISTIC, _hip.GRAM_SCORE, *[ctypes.c_void_p(x.data_ptr()) for x in t],
            None, None, off.ctypes.data_as(ctypes.c_void_p), 1, q, len(levels),
            lv.ctypes.data_as(ctypes.c_void_p), 1, None, None, ctypes.c_void_p(beta.data_ptr()),
            0, 0, ctypes.c_void_p(gram.data_ptr()), ctypes.c_void_p(gram[P * P:].data_ptr()),
            None, None, ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
        torch.cuda.synchronize()
        assert rc == want and text in _hip.last_error(), (shape[:2], rc, _hip.last_error())
        _untouched({"gram": out.cpu().numpy()})
