"""GPU: the row diagnostics pass (``glm_rows_batched``: eta, mu, the signed
residuals, leverages, Cook's distances) against the numpy yardstick
tests/_rows_ref.py, and ``dlsa_fit_sharded(cov_type="HC3")``.

Shapes: tests/test_gpu_gram.py's -- (p, intercept) through NT = ceil(P / 16) =
1 .. 12 with tile edges on both sides and odd p, and p = 128 (p = 0 mod 32,
where the tile phase's transposed read of the slot is at its worst);
partitions of (3001, 1500, 0, 4096, 1, 2003) rows in chunks of 1000.

Bounds: per row, tests/_rows_ref.py's (from the operations, pinned by
tests/test_cpu_rows.py).  The factor R of every information matrix is computed
once on the host (``models.rows_factor``) and given to both sides.
"""

import ctypes
import functools

import numpy as np
import pytest

import _glm_ref as G
import _gram_ref as GR
import _poison as PZ
import _rows_ref as RR

pytestmark = pytest.mark.gpu

SIZES, EMPTY, SINGLE, RPC = RR.SIZES, RR.EMPTY, RR.SINGLE, 1000
ALL = RR.STREAMS + ("cooks",)


@pytest.fixture(scope="module")
def M():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a visible MI355X"
    from dlsa_amd import models
    return models


def _host(g):
    return {k: v.cpu().numpy() for k, v in g.items()}


def _part_of(off):
    return np.repeat(np.arange(len(off) - 1), np.diff(off))


def _check(got, ref, bnd, off, R, what):
    """Every stream within its bound of the yardstick; the residuals' signs
    wherever the value exceeds its bound; NaN leverages exactly in the
    partitions whose factor is NaN.  Prints the figures before it asserts."""
    worst = {}
    worst["eta"] = RR.ratio(np.abs(got["eta"] - ref["eta"]), bnd["eta"])
    worst["mu"] = RR.ratio(np.abs(got["mu"] - ref["mu"]), bnd["mu"])
    for name, key in (("dev_res", "dev"), ("pearson_res", "chi")):
        worst[name] = RR.ratio(np.abs(got[name] ** 2 - np.maximum(ref[key], 0.0)), bnd[key])
        sure = np.abs(ref[key]) > bnd[key]
        assert np.array_equal(np.signbit(got[name])[sure], (ref["sign"] < 0)[sure]), (what, name)
    if "leverage" in got:
        part = _part_of(off)
        Rk = R[None].repeat(len(off) - 1, 0) if R.ndim == 2 else R
        nanrow = np.isnan(Rk).any(axis=(1, 2))[part]
        assert np.isnan(got["leverage"][nanrow]).all(), (what, "NaN factor, finite leverage")
        assert not np.isnan(got["leverage"][~nanrow]).any(), (what, "leverage NaN")
        worst["leverage"] = RR.ratio(np.abs(got["leverage"] - ref["leverage"])[~nanrow],
                                     bnd["leverage"][~nanrow])
        if "cooks" in got:
            h, r = got["leverage"], got["pearson_res"]
            with np.errstate(divide="ignore", invalid="ignore"):  # h = 1: one row at P = 1
                want = r * r * h / (Rk.shape[1] * (1.0 - h) ** 2)
            ok = ~nanrow
            assert np.allclose(got["cooks"][ok], want[ok], rtol=1e-14, atol=0, equal_nan=True)
    figs = {k: float(v.max(initial=0.0)) for k, v in worst.items()}
    print(what, " ".join(f"{k} {v:.3f}" for k, v in figs.items()), "(of the bound)")
    for k, v in figs.items():
        assert v <= 1.0, (what, k, v)


@pytest.mark.parametrize("p,fi,family,mask", RR.CASES, ids=RR.CASE_IDS)
def test_against_the_yardstick(M, monkeypatch, p, fi, family, mask):
    """Own thetas with own info, a shared beta with a shared info; with and
    without center / scale."""
    d = RR.dense(p, fi)
    o, w = RR.extras(d, mask)
    y, off, P, K = d[family], d["off"], p + fi, len(SIZES)
    for std in (False, True):
        Z = d["Zs"] if std else d["Z"]
        coef = d["thetas"] * (0.4 if std else 1.0)
        kw = dict(eta_offset=o, sample_weight=w, fit_intercept=fi, rows_per_chunk=RPC)
        if std:
            kw.update(center=d["center"], scale=d["scale"])
        S = RR.own_factors(family, Z, off, coef, w, o)
        for own in (True, False):
            sel = dict(thetas=coef) if own else dict(beta=coef[1])
            info = S if own else S[0]
            R = M.rows_factor(info, K, P)  # once, for both sides
            monkeypatch.setattr(M, "rows_factor", lambda *a, R=R: R)
            got = _host(M.glm_rows_batched(family, d["X"], y, off, info=info, **sel, **kw))
            monkeypatch.undo()
            assert set(got) == set(ALL) and all(v.shape == (int(off[-1]),) for v in got.values())
            ref, bnd = RR.partitions(family, Z, y, off, R=R, w=w, o=o, **sel)
            what = f"{family}-{mask} p={p} ic={int(fi)} std={int(std)} own={int(own)}"
            _check(got, ref, bnd, off, R, what)
            if own and P > 1:  # one row cannot carry P > 1 coefficients
                assert np.isnan(R[SINGLE]).all()


@pytest.mark.parametrize("p,fi,family,mask", [(33, False, "poisson", "both"),
                                              (100, True, "logistic", "wgt"),
                                              (128, False, "poisson", "both")],
                         ids=["p33-poisson", "p100-logistic", "p128-poisson"])
def test_bits_do_not_depend_on_the_chunking(M, p, fi, family, mask):
    import torch

    d = RR.dense(p, fi)
    o, w = RR.extras(d, mask)
    S = RR.own_factors(family, d["Z"], d["off"], d["thetas"], w, o)
    kw = dict(thetas=d["thetas"], info=S, eta_offset=o, sample_weight=w, fit_intercept=fi)
    first = M.glm_rows_batched(family, d["X"], d[family], d["off"], rows_per_chunk=0, **kw)
    for rpc in (0, 1000, 32, 33, 4097):
        g = M.glm_rows_batched(family, d["X"], d[family], d["off"], rows_per_chunk=rpc, **kw)
        for k in ALL:
            assert PZ.bits_equal(g[k].cpu().numpy(), first[k].cpu().numpy()), (rpc, k)
    part = M.glm_rows_batched(family, d["X"], d[family], d["off"], outputs=("mu", "dev_res"),
                              **dict(kw, info=None))
    assert set(part) == {"mu", "dev_res"}
    assert all(torch.equal(part[k], first[k]) for k in part), "without the tile phase"


# ---- buffers, padded rows and NaN rows: the C entry on a poisoned arena -------------------------

@pytest.mark.parametrize("family", ["logistic", "poisson"])
def test_buffers_and_nan_rows(M, family):
    """Inputs and outputs inside a 0xFF-filled arena with guard bands, X at an
    address that is 8 modulo 16 (NaN bytes behind it): every requested stream
    is written in [0, n) and nowhere else, an unrequested one keeps its
    pattern.  A NaN in the first row of partition 1 -- partition 0's last block
    holds it as padding -- in X, then in the weight, then in the offset: that
    row's outputs that depend on it are NaN, every other bit stays.  Then
    clean inputs after another pass used the workspace: the first run's bits."""
    import torch

    from dlsa_amd import _hip

    lib, stream = _hip.load(), torch.cuda.current_stream().cuda_stream
    fam = {"logistic": _hip.FAMILY_LOGISTIC, "poisson": _hip.FAMILY_POISSON}[family]
    d = RR.dense(15, True)
    has_o = family == "poisson"
    K, P, off = len(SIZES), 16, d["off"]
    n = int(off[-1])
    thetas = np.ascontiguousarray(d["thetas"])
    o, w = (d["o"] if has_o else None), d["w"]
    R = M.rows_factor(RR.own_factors(family, d["Z"], off, thetas, w, o), K, P)
    A = PZ.Arena(torch.device("cuda"))
    A.add("X", d["X"].nbytes, 16, 8).add("y", n * 8).add("o", n * 8).add("w", n * 8)
    A.add("thetas", thetas.nbytes).add("R", R.nbytes)
    for name in RR.STREAMS:
        A.add(name, n * 8)
    A.build()
    A.put("thetas", thetas)
    A.put("R", R)
    A.put("y", d[family])

    def run(X, ov, wv, skip=()):
        A.put("X", X)
        A.put("o", ov)
        A.put("w", wv)
        for name in RR.STREAMS:
            A.fill(name, PZ.POISON)
        ptr = lambda name: None if name in skip else A.ptr(name)
        rc = lib.dlsa_glm_rows_batched_chunked(
            fam, A.ptr("X"), A.ptr("y"), A.ptr("o") if has_o else None, A.ptr("w"),
            off.ctypes.data_as(ctypes.c_void_p), K, 15, 1, None, None, A.ptr("thetas"), P,
            None if "leverage" in skip else A.ptr("R"), P * P, RPC, *[ptr(s) for s in RR.STREAMS],
            stream)
        torch.cuda.synchronize()
        _hip.check(rc, "dlsa_glm_rows_batched_chunked")
        A.guards_intact()
        A.inputs_unchanged()
        for name in RR.STREAMS:
            if name in skip:
                assert (A.raw(name) == PZ.POISON).all(), (name, "an unrequested stream was written")
            else:
                A.fully_written(name, np.float64)
        return {s: A.get(s, np.float64) for s in RR.STREAMS if s not in skip}

    clean = run(d["X"], d["o"], d["w"])
    ref, bnd = RR.partitions(family, d["Z"], d[family], off, thetas=thetas, R=R, w=w, o=o)
    _check(clean, ref, bnd, off, R, f"arena {family}")
    for skip in (("leverage",), ("eta", "dev_res"), ("mu", "pearson_res", "leverage")):
        some = run(d["X"], d["o"], d["w"], skip)
        assert all(PZ.bits_equal(some[s], clean[s]) for s in some), skip

    a = int(off[1])  # partition 1's first row: padding of partition 0's last block
    watch = [a - 1, a - 2, int(off[SINGLE]), int(off[SINGLE]) - 1, int(off[SINGLE]) + 1, n - 1]
    poisons = [("X", RR.STREAMS), ("w", ("dev_res", "pearson_res", "leverage"))]
    if has_o:
        poisons.append(("o", RR.STREAMS))
    for which, hit in poisons:
        X, ov, wv = d["X"].copy(), d["o"].copy(), d["w"].copy()
        if which == "X":
            X[a, 7] = np.nan
        else:
            (ov if which == "o" else wv)[a] = np.nan
        bad = run(X, ov, wv)
        for s in RR.STREAMS:
            assert np.isnan(bad[s][a]) == (s in hit), (which, s)
            rest = np.ones(n, bool)
            rest[a] = s not in hit
            assert PZ.bits_equal(bad[s][rest], clean[s][rest]), (which, s, "another row changed")
            assert PZ.bits_equal(bad[s][watch], clean[s][watch])

    # another pass leaves its image in the stream-ordered workspace
    M.glm_gram_batched(family, d["X"], d[family], off, thetas=thetas, sample_weight=d["w"],
                       fit_intercept=True, rows_per_chunk=RPC)
    again = run(d["X"], d["o"], d["w"])
    for s in RR.STREAMS:
        assert PZ.bits_equal(again[s], clean[s]), s


def test_bad_info_is_nan_in_its_partition_only(M):
    d = RR.dense(16, True)
    off, P = d["off"], 17
    S = RR.own_factors("logistic", d["Z"], off, d["thetas"], d["w"])
    kw = dict(thetas=d["thetas"], sample_weight=d["w"], fit_intercept=True, rows_per_chunk=RPC)
    good = _host(M.glm_rows_batched("logistic", d["X"], d["logistic"], off, info=S, **kw))
    S2 = S.copy()
    S2[1] = -S2[1]       # not positive definite
    S2[3, 5, 2] = np.nan
    bad = _host(M.glm_rows_batched("logistic", d["X"], d["logistic"], off, info=S2, **kw))
    part = _part_of(off)
    hit = np.isin(part, (1, 3))
    for s in ALL:
        if s in ("leverage", "cooks"):
            assert np.isnan(bad[s][hit]).all(), s
            assert PZ.bits_equal(bad[s][~hit], good[s][~hit]), s
        else:
            assert PZ.bits_equal(bad[s], good[s]), s
    assert np.isnan(good["leverage"][part == SINGLE]).all()  # one row, P = 17
    assert not np.isnan(good["leverage"][np.isin(part, (0, 1, 3, 5))]).any()
    # only empty partitions: a no-op
    e = M.glm_rows_batched("logistic", d["X"][:0], d["logistic"][:0], np.zeros(3, np.int64),
                           thetas=d["thetas"][:2], info=S[:2], fit_intercept=True)
    assert all(v.shape == (0,) for v in e.values())


@pytest.mark.parametrize("family,p", [("poisson", 13), ("logistic", 13), ("poisson", 100),
                                      ("logistic", 100)])
def test_leverages_of_a_fit_sum_to_p(M, family, p):
    """At the fit's own theta and sig_inv: sum h = P within 1e-9 P over every
    converged partition, 0 <= h < 1, and a row of weight 0 has h = 0 and a
    finite mu."""
    sizes = (3001, 1500, 0, 2003)
    d = RR.dense(p, True, sizes)
    y, off, P = d[family], d["off"], p + 1
    if family == "poisson":
        kw = dict(sample_weight=d["w"], eta_offset=d["o"], fit_intercept=True)
        fit = M.poisson_model_batched_weighted(d["X"], y, off, **kw)
        w = d["w"]
    else:
        kw = dict(fit_intercept=True)
        fit = M.logistic_model_batched(d["X"], y, off, **kw)
        w = np.ones(len(y))
    assert fit.status.cpu().tolist() == [0, 0, 3, 0]
    g = _host(M.glm_rows_batched(family, d["X"], y, off, thetas=fit.theta, info=fit.sig_inv, **kw))
    part = _part_of(off)
    for k in (0, 1, 3):
        h = g["leverage"][part == k]
        print(f"{family} P={P} partition {k}: sum h - P = {h.sum() - P:.3e}, max h {h.max():.4f}")
        assert abs(h.sum() - P) <= 1e-9 * P, (k, h.sum())
        assert (h >= 0).all() and (h < 1).all()
    zero = w == 0
    assert zero.sum() > 0 or family == "logistic"
    assert not g["leverage"][zero].any() and np.isfinite(g["mu"][zero]).all()
    assert np.isfinite(g["cooks"]).all()


def test_fit_sharded_hc3(M):
    """cov_type="HC3" on over-dispersed counts, K = 8 partitions of 400 rows,
    p = 4 and an intercept: cov within 1e-8 of the yardstick's A^-1 M_HC3 A^-1
    (leverages against each partition's own sig_inv), std_err at least HC0's,
    wlse the plain run's to the bit."""
    from dlsa_amd.distributed import dlsa_fit_sharded

    X, y, off = GR.negbin_job(3, K=8, n_k=400, p=4)
    kw = dict(fit_intercept=True, family="poisson")
    plain = dlsa_fit_sharded(X, y, off, **kw)
    hc0 = dlsa_fit_sharded(X, y, off, cov_type="HC0", **kw)
    hc3 = dlsa_fit_sharded(X, y, off, cov_type="HC3", **kw)
    fit = plain["fit"]
    assert fit.status.cpu().tolist() == [0] * 8
    th, Sk = fit.theta.cpu().numpy(), fit.sig_inv.cpu().numpy()
    Z, P = G.design(X, True), 5
    R = M.rows_factor(Sk, 8, P)
    Mref = np.zeros((P, P))
    for k, (a, b) in enumerate(zip(off[:-1], off[1:])):
        h = RR.rows("poisson", Z[a:b], y[a:b], th[k], R[k])["leverage"]
        assert (h < 1).all()
        Mref += RR.hc3_meat("poisson", Z[a:b], y[a:b], th[k], h)
    cov_ref, _ = GR.sandwich(plain["Sig_inv_sum"], Mref)
    rel = lambda a, b: float(np.abs(a - b).max() / np.abs(b).max())
    figs = (rel(hc3["meat_sum"], Mref), rel(hc3["cov"], cov_ref))
    print("HC3 meat cov", " ".join(f"{v:.2e}" for v in figs),
          "std_err HC3 / HC0", np.round(hc3["std_err"] / hc0["std_err"], 4))
    assert max(figs) <= 1e-8, figs
    assert set(hc3) == set(hc0)
    assert (hc3["std_err"] >= hc0["std_err"]).all()
    assert PZ.bits_equal(hc3["wlse"], plain["wlse"])
    assert PZ.bits_equal(hc0["wlse"], plain["wlse"])


def test_error_codes(M):
    """P = 193: DLSA_E_UNSUPPORTED before any launch (the outputs keep their
    poison); leverage without rfac and a bad rfac stride: DLSA_E_INVALID."""
    import torch

    from dlsa_amd import _hip
    from dlsa_amd._hip import DlsaHipError

    n = 64
    X, y, off = np.zeros((n, 193)), np.zeros(n), np.array([0, n])
    with pytest.raises(DlsaHipError, match=r"\(-3\)"):
        M.glm_rows_batched("logistic", X, y, off, beta=np.zeros(193))
    with pytest.raises(DlsaHipError, match=r"\(-3\)"):
        M.glm_rows_batched("poisson", X[:, :192], y, off, beta=np.zeros(193), fit_intercept=True,
                           info=np.eye(193))
    lib, stream = _hip.load(), torch.cuda.current_stream().cuda_stream
    Xd = torch.zeros((n, 3), dtype=torch.float64, device="cuda")
    v = torch.zeros(n, dtype=torch.float64, device="cuda")
    out = torch.full((n,), float("nan"), dtype=torch.float64, device="cuda")
    offs = np.array([0, n], dtype=np.int64)

    def call(family=_hip.FAMILY_POISSON, o=None, stride=0, rfac=v.data_ptr(), rstride=0):
        return lib.dlsa_glm_rows_batched(family, Xd.data_ptr(), v.data_ptr(), o, None,
                                         offs.ctypes.data_as(ctypes.c_void_p), 1, 3, 0, None, None,
                                         v.data_ptr(), stride, rfac, rstride, out.data_ptr(),
                                         out.data_ptr(), None, None, out.data_ptr(), stream)

    assert call(stride=2) == -1
    assert call(rstride=3) == -1
    assert call(rfac=None) == -1
    assert call(family=_hip.FAMILY_LOGISTIC, o=v.data_ptr()) == -1
    assert call(family=1) == -3
    torch.cuda.synchronize()
    assert torch.isnan(out).all()
