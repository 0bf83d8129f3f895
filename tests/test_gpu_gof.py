"""GPU: the goodness-of-fit pass (deviance, Pearson chi-square, rows with a
positive weight) on the dense and the categorical-code layout, against the
numpy yardstick tests/_gof_ref.py.

Shapes are the smallest at which the kernels can go wrong: partitions of
(1000, 31, 0, 2049) rows -- a tail block, a partition shorter than one block,
an empty one, one row past a block multiple (of the dense pass's 32 and the
code pass's 256) -- odd p, whose rows straddle the 16-byte pieces of the ring,
p = 200 for the multi-piece slots, and B = 1, the most candidates of a pass and
three more (two passes).

Tolerance: every entry of ``deviance`` and ``pearson`` within 1e-12 relative of
the yardstick's entry, the bound of the log-likelihood evaluation tests.  On
the CPU, at n = 7704, p = 10, y up to 351, the cancelling and the
cancellation-free forms and sequential against exactly rounded summation agree
to better than 1e-15 relative, which leaves about three orders of magnitude
for the device's exp / log and its summation order.  ``n_pos`` is exact.  The
candidates keep |eta| <= 20.
"""

import ctypes
import functools

import numpy as np
import pytest

import _glm_ref as G
import _gof_ref as R
import _poison as PZ

pytestmark = pytest.mark.gpu

REL = 1e-12
SIZES = (1000, 31, 0, 2049)
EMPTY = 2
FAMILY_MASKS = [("logistic", "none"), ("logistic", "wgt"), ("poisson", "none"),
                ("poisson", "ofs"), ("poisson", "wgt"), ("poisson", "both")]
FM_IDS = [f"{f}-{m}" for f, m in FAMILY_MASKS]


@pytest.fixture(scope="module")
def M():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a visible MI355X"
    from dlsa_amd import models
    return models


def _offsets(sizes):
    return np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)


@functools.lru_cache(maxsize=None)
def _dense(p, fi, sizes=SIZES):
    """X, the two families' y, offset, weights, offsets and B candidates (the
    most of a pass + 3) with |eta| <= 20, once per process."""
    import oracle as O
    from dlsa_amd import _hip

    off = _offsets(sizes)
    n = int(off[-1])
    X, ylog = O.simulate_counter(n, p, seed=40 + p)
    X = np.ascontiguousarray(X)
    rng = np.random.default_rng(p)
    o = rng.uniform(np.log(0.2), np.log(5.0), n)
    star = np.concatenate([[1.0] * fi, rng.uniform(-1, 1, p) * 2.0 / np.sqrt(p)])
    Z = G.design(X, fi)
    ypois = rng.poisson(np.exp(Z @ star + o)).astype(np.float64)
    B = _hip.MAX_GOF_CANDIDATES + 3
    betas = star + rng.standard_normal((B, p + fi)) * 2.0 / np.sqrt(p + fi)
    betas[0] = star
    assert np.abs(Z @ betas.T).max() + np.abs(o).max() <= 20.0
    w = G.weights(n, "real")
    for a in (X, ylog, ypois, o, w, betas):
        a.setflags(write=False)
    return dict(X=X, logistic=np.ascontiguousarray(ylog), poisson=ypois, o=o, w=w, off=off,
                betas=betas, Z=Z)


def _extras(d, mask):
    return (d["o"] if mask in ("ofs", "both") else None,
            d["w"] if mask in ("wgt", "both") else None)


def _host(g):
    return {k: v.cpu().numpy() for k, v in g.items()}


def _check(got, want, what):
    """Every entry within REL of the yardstick's; n_pos exact; prints the
    figures before it asserts."""
    dev, chi, npos = want
    for name, a, b in (("deviance", got["deviance"], dev), ("pearson", got["pearson"], chi)):
        assert a.shape == b.shape, (what, name, a.shape, b.shape)
        nz = b != 0
        assert not a[~nz].view(np.uint64).any(), (what, name, "an empty partition is exactly 0")
        e = float((np.abs(a[nz] - b[nz]) / np.abs(b[nz])).max()) if nz.any() else 0.0
        print(f"{what} {name}: max relative error {e:.3e}")
        assert e <= REL, (what, name, e)
    assert got["n_pos"].dtype == np.int64 and got["n_pos"].tolist() == npos.tolist(), what


def _check_sums(got, what):
    for name in ("deviance", "pearson"):
        acc = np.zeros(got[name].shape[1])
        for row in got[name]:  # k ascending
            acc = acc + row
        assert PZ.bits_equal(got[name + "_sum"], acc), (what, name)
    assert int(got["n_pos_sum"]) == int(got["n_pos"].sum()), what


# ---- dense layout ----------------------------------------------------------------------------

@pytest.mark.parametrize("fm", FAMILY_MASKS, ids=FM_IDS)
@pytest.mark.parametrize("p,fi", [(3, False), (3, True), (13, False), (13, True)])
def test_dense_against_the_yardstick(M, p, fi, fm):
    """Every kernel the pass instantiates, B = 1, the most of a pass and three
    more (grouping), two calls bit-identical."""
    import torch

    family, mask = fm
    d = _dense(p, fi)
    o, w = _extras(d, mask)
    y, off = d[family], d["off"]
    want = R.gof_partitions(family, d["Z"], y, off, betas=d["betas"], w=w, o=o)
    kw = dict(eta_offset=o, sample_weight=w, fit_intercept=fi, return_sum=True)
    for B in (1, M.MAX_GOF_CANDIDATES, M.MAX_GOF_CANDIDATES + 3):
        g = M.glm_gof_batched(family, d["X"], y, off, betas=d["betas"][:B], **kw)
        g2 = M.glm_gof_batched(family, d["X"], y, off, betas=d["betas"][:B], **kw)
        assert all(torch.equal(g[k], g2[k]) for k in g), "two calls differ"
        got = _host(g)
        what = f"dense {family}-{mask} p={p} ic={fi} B={B}"
        _check(got, (want[0][:, :B], want[1][:, :B], want[2]), what)
        _check_sums(got, what)


def test_dense_multi_piece_slots_and_standardised(M):
    """p = 200 (P > 192: slots of several pieces per wave), and center / scale."""
    d = _dense(200, True, (257, 64))
    for family, mask in (("logistic", "wgt"), ("poisson", "both")):
        o, w = _extras(d, mask)
        want = R.gof_partitions(family, d["Z"], d[family], d["off"], betas=d["betas"][:3], w=w,
                                o=o)
        got = _host(M.glm_gof_batched(family, d["X"], d[family], d["off"], betas=d["betas"][:3],
                                      eta_offset=o, sample_weight=w, fit_intercept=True))
        _check(got, want, f"dense p=200 {family}-{mask}")
    d = _dense(13, True)
    c, s = d["X"].mean(0), d["X"].std(0, ddof=1) * 0.5
    Z = G.design(d["X"], True, c, s)
    betas = d["betas"][:4] * 0.4  # scale halves: |eta| stays <= 20
    assert np.abs(Z @ betas.T).max() + np.abs(d["o"]).max() <= 20.0
    want = R.gof_partitions("poisson", Z, d["poisson"], d["off"], betas=betas, w=d["w"], o=d["o"])
    got = _host(M.glm_gof_batched("poisson", d["X"], d["poisson"], d["off"], betas=betas,
                                  eta_offset=d["o"], sample_weight=d["w"], fit_intercept=True,
                                  center=c, scale=s))
    _check(got, want, "dense standardised")


def test_dense_per_partition_mode(M):
    """thetas from a fit: row k is what shared mode gives with betas =
    thetas[k:k+1] in row k, bit for bit -- and the yardstick's value."""
    import torch

    d = _dense(3, True)
    y, off = d["poisson"], d["off"]
    fit = M.poisson_model_batched_weighted(d["X"], y, off, sample_weight=d["w"],
                                           eta_offset=d["o"], fit_intercept=True)
    assert fit.status.cpu().tolist()[EMPTY] == 3
    kw = dict(eta_offset=d["o"], sample_weight=d["w"], fit_intercept=True)
    per = M.glm_gof_batched("poisson", d["X"], y, off, thetas=fit.theta, **kw)
    th = fit.theta.cpu().numpy()
    want = R.gof_partitions("poisson", d["Z"], y, off, thetas=th, w=d["w"], o=d["o"])
    _check(_host(per), want, "dense per-partition")
    for k in range(len(SIZES)):
        sh = M.glm_gof_batched("poisson", d["X"], y, off, betas=fit.theta[k:k + 1], **kw)
        for name in ("deviance", "pearson"):
            assert torch.equal(per[name][k], sh[name][k]), (name, k)
    with pytest.raises(ValueError, match="thetas must be"):
        M.glm_gof_batched("poisson", d["X"], y, off, thetas=th[:2], **kw)


# ---- categorical-code layout --------------------------------------------------------------------

CAT_NUMERIC, CAT_FACTORS = 5, (4, 6, 3)


@functools.lru_cache(maxsize=None)
def _cat():
    """A reduced airline-like shape from ``simulate_categorical`` (5 numeric
    columns, factors of 4, 6 and 3 levels, intercept: P = 16), the partition
    sizes of the dense tests, Poisson counts drawn here."""
    import torch

    from dlsa_amd import models as M

    off = _offsets(SIZES)
    n = int(off[-1])
    Xn, codes, ylog, levels = M.simulate_categorical(n, seed=77, numeric=CAT_NUMERIC,
                                                     factors=CAT_FACTORS, device="cpu")
    Xn, codes, ylog = Xn.numpy(), codes.numpy(), ylog.numpy()
    Xd = M.expand_categorical(torch.from_numpy(Xn), torch.from_numpy(codes), levels).numpy()
    Z = G.design(Xd, True)
    rng = np.random.default_rng(8)
    P = Z.shape[1]
    star = np.concatenate([[0.8], rng.uniform(-1, 1, P - 1) * 0.6])
    o = rng.uniform(np.log(0.2), np.log(5.0), n)
    ypois = rng.poisson(np.exp(Z @ star + o)).astype(np.float64)
    B = M.MAX_GOF_CANDIDATES + 3
    betas = star + rng.standard_normal((B, P)) * 0.5
    betas[0] = star
    assert np.abs(Z @ betas.T).max() + np.abs(o).max() <= 20.0
    return dict(Xn=Xn, codes=codes, levels=[int(v) for v in levels], logistic=ylog, poisson=ypois,
                o=o, w=G.weights(n, "real"), off=off, betas=betas, Z=Z, Xd=Xd)


@pytest.mark.parametrize("fm", FAMILY_MASKS, ids=FM_IDS)
def test_categorical_against_the_yardstick_and_the_dense_kernel(M, fm):
    import torch

    family, mask = fm
    d = _cat()
    o, w = _extras(d, mask)
    y, off = d[family], d["off"]
    want = R.gof_partitions(family, d["Z"], y, off, betas=d["betas"], w=w, o=o)
    kw = dict(eta_offset=o, sample_weight=w, fit_intercept=True, return_sum=True)
    for B, rpc in ((1, 0), (M.MAX_GOF_CANDIDATES, 700), (M.MAX_GOF_CANDIDATES + 3, 0)):
        b = d["betas"][:B]
        g = M.glm_gof_batched_categorical(family, d["Xn"], d["codes"], y, off, d["levels"],
                                          betas=b, rows_per_chunk=rpc, **kw)
        g2 = M.glm_gof_batched_categorical(family, d["Xn"], d["codes"], y, off, d["levels"],
                                           betas=b, rows_per_chunk=rpc, **kw)
        assert all(torch.equal(g[k], g2[k]) for k in g), "two calls differ"
        got = _host(g)
        what = f"cat {family}-{mask} B={B}"
        _check(got, (want[0][:, :B], want[1][:, :B], want[2]), what)
        _check_sums(got, what)
        dense = _host(M.glm_gof_batched(family, d["Xd"], y, off, betas=b, **kw))
        _check(got, (dense["deviance"], dense["pearson"], dense["n_pos"]), what + " vs dense")


def test_categorical_per_partition_mode_and_bad_code(M):
    import torch

    from dlsa_amd._hip import DlsaHipError

    d = _cat()
    y, off = d["poisson"], d["off"]
    thetas = np.ascontiguousarray(d["betas"][:len(SIZES)])
    args = ("poisson", d["Xn"], d["codes"], y, off, d["levels"])
    kw = dict(eta_offset=d["o"], sample_weight=d["w"], fit_intercept=True)
    per = M.glm_gof_batched_categorical(*args, thetas=thetas, **kw)
    want = R.gof_partitions("poisson", d["Z"], y, off, thetas=thetas, w=d["w"], o=d["o"])
    _check(_host(per), want, "cat per-partition")
    for k in range(len(SIZES)):
        sh = M.glm_gof_batched_categorical(*args, betas=thetas[k:k + 1], **kw)
        for name in ("deviance", "pearson"):
            assert torch.equal(per[name][k], sh[name][k]), (name, k)
    codes = d["codes"].copy()
    codes[1500, 1] = d["levels"][1]
    with pytest.raises(DlsaHipError, match="level codes"):
        M.glm_gof_batched_categorical("poisson", d["Xn"], codes, y, off, d["levels"],
                                      betas=d["betas"][:2], **kw)


# ---- buffers and padded rows: the C entries on a poisoned arena ---------------------------------

def _c_call(lib, stream, A, layout, fam, d, B, has_o):
    """The C entry of ``layout`` on the arena's regions (shared candidates,
    intercept, no standardisation); waits for it."""
    import torch

    offp = d["off"].ctypes.data_as(ctypes.c_void_p)
    K = len(d["off"]) - 1
    o = A.ptr("o") if has_o else None
    outs = (A.ptr("dev"), A.ptr("chi"), A.ptr("npos"), A.ptr("sums"), stream)
    if layout == "dense":
        rc = lib.dlsa_glm_gof_batched(fam, A.ptr("X"), A.ptr("y"), o, A.ptr("w"), offp, K,
                                      d["X"].shape[1], 1, None, None, A.ptr("betas"), B, 0, *outs)
    else:
        lv = np.asarray(d["levels"], dtype=np.int32)
        rc = lib.dlsa_glm_gof_categorical(fam, A.ptr("X"), A.ptr("codes"), A.ptr("y"), o,
                                          A.ptr("w"), offp, K, d["Xn"].shape[1], len(lv),
                                          lv.ctypes.data_as(ctypes.c_void_p), 1, None, None,
                                          A.ptr("betas"), B, 0, 700, *outs)
    torch.cuda.synchronize()
    return rc


@pytest.mark.parametrize("family", ["logistic", "poisson"])
@pytest.mark.parametrize("layout", ["dense", "cat"])
def test_buffers_and_padded_rows(M, layout, family):
    """Inputs and outputs inside a 0xFF-filled arena with guard bands (X at an
    address that is 8 modulo 16), the outputs poisoned: nothing outside the
    outputs is written and no output entry is left unwritten.  Then NaN in the
    weight, offset and y of partition 1's first row -- the row just past
    partition 0's end, which partition 0's last block (1000 = 31 x 32 + 8 rows)
    holds as padding: only partition 1's sums become non-finite, every other
    entry keeps its bits."""
    import torch

    from dlsa_amd import _hip

    lib, stream = _hip.load(), torch.cuda.current_stream().cuda_stream
    fam = {"logistic": _hip.FAMILY_LOGISTIC, "poisson": _hip.FAMILY_POISSON}[family]
    d = _dense(13, True) if layout == "dense" else _cat()
    X = d["X"] if layout == "dense" else d["Xn"]
    has_o = family == "poisson"
    B, K = 3, len(SIZES)
    betas = np.ascontiguousarray(d["betas"][:B])
    y, o, w = d[family].copy(), d["o"].copy(), d["w"].copy()
    A = PZ.Arena(torch.device("cuda"))
    A.add("X", X.nbytes, 16, 8).add("y", y.nbytes).add("o", o.nbytes).add("w", w.nbytes)
    if layout == "cat":
        A.add("codes", d["codes"].nbytes)
    A.add("betas", betas.nbytes)
    A.add("dev", K * B * 8).add("chi", K * B * 8).add("npos", K * 8).add("sums", (2 * B + 1) * 8)
    A.build()
    A.put("X", X)
    A.put("betas", betas)
    if layout == "cat":
        A.put("codes", d["codes"])
    runs = []
    for nan_row in (None, int(d["off"][1])):
        if nan_row is not None:
            y[nan_row] = o[nan_row] = w[nan_row] = np.nan
        A.put("y", y)
        A.put("o", o)
        A.put("w", w)
        for name in ("dev", "chi", "npos", "sums"):
            A.fill(name, PZ.POISON)
        rc = _c_call(lib, stream, A, layout, fam, d, B, has_o)
        _hip.check(rc, f"gof {layout}")
        A.guards_intact()
        A.inputs_unchanged()
        for name in ("dev", "chi", "npos", "sums"):
            A.fully_written(name, np.float64)
        runs.append(dict(deviance=A.get("dev", np.float64, (K, B)),
                         pearson=A.get("chi", np.float64, (K, B)),
                         n_pos=A.get("npos", np.float64).astype(np.int64),
                         sums=A.get("sums", np.float64)))
    clean, bad = runs
    want = R.gof_partitions(family, d["Z"], d[family], d["off"], betas=betas, w=d["w"],
                            o=d["o"] if has_o else None)
    _check(clean, want, f"arena {layout} {family}")
    assert np.isfinite(clean["sums"]).all() and clean["sums"][-1] == want[2].sum()
    for name in ("deviance", "pearson"):
        assert not np.isfinite(bad[name][1]).any(), name
        for k in (0, 2, 3):
            assert PZ.bits_equal(bad[name][k], clean[name][k]), (name, k)
    assert not np.isfinite(bad["sums"][:2 * B]).any()
    # the NaN weight is not > 0: partition 1 counts one row fewer
    assert (clean["n_pos"] - bad["n_pos"]).tolist() == [0, int(d["w"][d["off"][1]] > 0), 0, 0]


# ---- sharded ----------------------------------------------------------------------------------------

def test_gof_sharded_without_a_group_is_the_local_totals(M):
    from dlsa_amd.distributed import gof_sharded

    B = M.MAX_GOF_CANDIDATES + 3
    d, c = _dense(13, True), _cat()
    kw = dict(fit_intercept=True, eta_offset=d["o"], sample_weight=d["w"])
    tot = gof_sharded(d["X"], d["poisson"], d["off"], d["betas"][:B], family="poisson", **kw)
    g = _host(M.glm_gof_batched("poisson", d["X"], d["poisson"], d["off"], betas=d["betas"][:B],
                                return_sum=True, **kw))
    kw = dict(fit_intercept=True, sample_weight=c["w"])
    totc = gof_sharded(c["Xn"], c["logistic"], c["off"], c["betas"][:B], codes=c["codes"],
                       levels=c["levels"], **kw)
    gc = _host(M.glm_gof_batched_categorical("logistic", c["Xn"], c["codes"], c["logistic"],
                                             c["off"], c["levels"], betas=c["betas"][:B],
                                             return_sum=True, **kw))
    for t, h in ((tot, g), (totc, gc)):
        assert t["deviance"].shape == (B,)
        assert PZ.bits_equal(t["deviance"], h["deviance_sum"])
        assert PZ.bits_equal(t["pearson"], h["pearson_sum"])
        assert t["n_pos"] == int(h["n_pos_sum"]) == int(h["n_pos"].sum())


@functools.lru_cache(maxsize=None)
def _negbin():
    """Over-dispersed counts: y ~ NB(mean mu, size 2), Var y = mu (1 + mu / 2)."""
    sizes = (3000, 2500, 0, 3500)
    off = _offsets(sizes)
    n, p, r = int(off[-1]), 5, 2.0
    rng = np.random.default_rng(33)
    X = rng.standard_normal((n, p)) * 0.4
    theta = np.array([1.0, 0.5, -0.3, 0.0, 0.0, 0.25])
    mu = np.exp(G.design(X, True) @ theta)
    return X, rng.negative_binomial(r, r / (r + mu)).astype(np.float64), off


def test_dispersion_pearson(M):
    import warnings

    from dlsa_amd.distributed import dlsa_fit_sharded, finish
    from dlsa_amd.dlsa import reduce_partitions_device, split_reduced

    X, y, off = _negbin()
    kw = dict(fit_intercept=True, family="poisson")
    plain = dlsa_fit_sharded(X, y, off, **kw)
    none = dlsa_fit_sharded(X, y, off, dispersion=None, **kw)
    assert "dispersion" not in none and set(none) == set(plain)
    for key in ("wlse", "oneshot", "beta_byAIC", "beta_byBIC", "dbic_support", "Sig_inv_sum"):
        assert PZ.bits_equal(np.asarray(none[key], np.float64), np.asarray(plain[key], np.float64))
    for key in ("AIC", "BIC", "beta"):
        assert PZ.bits_equal(none["path"][key], plain["path"][key]), key

    out = dlsa_fit_sharded(X, y, off, dispersion="pearson", **kw)
    fit = out["fit"]
    P = fit.P
    th, st = fit.theta.cpu().numpy(), fit.status.cpu().numpy()
    assert st.tolist() == [0, 0, 3, 0]
    _, chi, npos = R.gof_partitions("poisson", G.design(X, True), y, off, thetas=th)
    phi = R.dispersion(chi[:, 0], npos, P, st <= 1)
    print(f"dispersion {out['dispersion']:.6f} yardstick {phi:.6f}")
    assert phi > 1.5 and abs(out["dispersion"] / phi - 1.0) <= 1e-10
    # the WLSE is lstsq(S / phi, v / phi): the plain run's to the solver's
    # rounding, cond(S) eps (a factor 100 for its constant)
    S = plain["Sig_inv_sum"]
    bound = 100 * np.linalg.cond(S) * np.finfo(np.float64).eps * np.abs(plain["wlse"]).max()
    assert np.abs(out["wlse"] - plain["wlse"]).max() <= bound
    # LARS / DBIC: finish on the plain run's reduced sums divided by that phi
    b = reduce_partitions_device(plain["fit"], n_rows=True).cpu().numpy()
    Sr, v, sth, K = split_reduced(b[:-1], P)
    want = finish(Sr / out["dispersion"], v / out["dispersion"], sth, K, int(round(b[-1])), True,
                  "lasso")
    for key in ("wlse", "beta_byAIC", "beta_byBIC", "dbic_support", "Sig_inv_sum"):
        assert PZ.bits_equal(np.asarray(out[key], np.float64), np.asarray(want[key], np.float64))
    assert PZ.bits_equal(out["path"]["BIC"], want["path"]["BIC"])
    # as many rows as parameters: no residual degrees of freedom
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        with pytest.raises(ValueError, match="degrees of freedom"):
            dlsa_fit_sharded(X[:6], y[:6], [0, 6], dispersion="pearson", **kw)
