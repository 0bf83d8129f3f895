"""GPU: the score outer-product pass (``glm_gram_batched``: the sandwich's meat
or the information matrix, and the score vector) against the numpy yardstick
tests/_gram_ref.py, and the robust covariance of ``dlsa_fit_sharded``.

Shapes: (p, intercept) through NT = ceil(P / 16) = 1 .. 12 with tile edges on
both sides and odd p (rows that start 8 modulo 16); partitions of (3001, 1500,
0, 4096, 1, 2003) rows in chunks of 1000 -- several chunks per partition whose
block tails and chunk tails differ, an empty partition, one of a single row.

Tolerance: every entry of a partition's ``gram`` within 1e-10 of the yardstick
relative to the block's largest entry, the project's per-entry bound for fp64
Gram sums; ``score`` within 1e-10 relative to max |Z|^T |s|.
"""

import ctypes
import functools
import os

import numpy as np
import pytest

import _glm_ref as G
import _gram_ref as R
import _poison as PZ

pytestmark = pytest.mark.gpu

REL = 1e-10
SIZES = (3001, 1500, 0, 4096, 1, 2003)
EMPTY = 2
RPC = 1000
SMALL = [(1, False), (1, True), (15, True), (16, True), (33, False)]
LARGE = [(100, True), (127, True), (129, False), (191, True), (192, False)]
FAMILY_MASKS = [("logistic", "none"), ("logistic", "wgt"), ("poisson", "none"),
                ("poisson", "ofs"), ("poisson", "wgt"), ("poisson", "both")]
CASES = [(p, fi, f, m) for p, fi in SMALL for f, m in FAMILY_MASKS] + \
        [(p, fi, f, m) for p, fi in LARGE for f, m in (("logistic", "wgt"), ("poisson", "both"))]
CASE_IDS = [f"p{p}-ic{int(fi)}-{f}-{m}" for p, fi, f, m in CASES]


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
    """X, the two families' y, offset, weights, offsets, per-partition thetas
    and one shared beta with |eta| <= 12, center / scale, once per process."""
    import oracle as O

    off = _offsets(sizes)
    n, K, P = int(off[-1]), len(sizes), p + fi
    X, _ = O.simulate_counter(n, p, seed=60 + p)
    X = np.ascontiguousarray(X)
    rng = np.random.default_rng(p)
    o = rng.uniform(np.log(0.2), np.log(5.0), n)
    star = np.concatenate([[0.5] * fi, rng.uniform(-1, 1, p) * 1.5 / np.sqrt(p)])
    Z = G.design(X, fi)
    ypois = rng.poisson(np.exp(Z @ star + o)).astype(np.float64)
    ylog = (rng.uniform(size=n) < G._expit(Z @ star)).astype(np.float64)
    thetas = star + rng.standard_normal((K, P)) * 0.5 / np.sqrt(P)
    c, s = X.mean(0), X.std(0, ddof=1) * 0.5 + 0.1
    Zs = G.design(X, fi, c, s)
    for z, scale in ((Z, 1.0), (Zs, 0.4)):
        assert np.abs(z @ (thetas * scale).T).max() + np.abs(o).max() <= 12.0
    w = G.weights(n, "real")
    for a in (X, ylog, ypois, o, w, thetas, Z, Zs):
        a.setflags(write=False)
    return dict(X=X, logistic=ylog, poisson=ypois, o=o, w=w, off=off, thetas=thetas, Z=Z, Zs=Zs,
                center=c, scale=s)


def _extras(d, mask):
    return (d["o"] if mask in ("ofs", "both") else None,
            d["w"] if mask in ("wgt", "both") else None)


def _host(g):
    return {k: v.cpu().numpy() for k, v in g.items()}


def _check(got, want, what):
    """gram per block within REL of its largest entry, score within REL of max
    |Z|^T |s|; exact symmetry; an empty partition exactly zero.  Prints the
    figures before it asserts."""
    Gw, sw, scale = want
    worst_g = worst_s = 0.0
    for k in range(Gw.shape[0]):
        a, b = got["gram"][k], Gw[k]
        assert np.array_equal(a, a.T), (what, k, "gram is not exactly symmetric")
        if not b.any():
            assert not a.view(np.uint64).any() and not got["score"][k].view(np.uint64).any(), \
                (what, k, "an empty partition is exactly 0")
            continue
        worst_g = max(worst_g, float(np.abs(a - b).max() / np.abs(b).max()))
        if scale[k] > 0:
            worst_s = max(worst_s, float(np.abs(got["score"][k] - sw[k]).max() / scale[k]))
    print(f"{what}: gram {worst_g:.3e} score {worst_s:.3e}")
    assert worst_g <= REL, (what, "gram", worst_g)
    assert worst_s <= REL, (what, "score", worst_s)


def _check_sums(got, what):
    for name in ("gram", "score"):
        acc = np.zeros(got[name].shape[1:])
        for blk in got[name]:  # k ascending
            acc = acc + blk
        assert PZ.bits_equal(got[name + "_sum"], acc), (what, name + "_sum")


@pytest.mark.parametrize("p,fi,family,mask", CASES, ids=CASE_IDS)
def test_against_the_yardstick(M, p, fi, family, mask):
    """Both kinds, at own thetas and at a shared beta, with and without
    center / scale; two calls bit-identical; the sums over k."""
    import torch

    d = _dense(p, fi)
    o, w = _extras(d, mask)
    y, off = d[family], d["off"]
    for std in (False, True):
        Z = d["Zs"] if std else d["Z"]
        coef = d["thetas"] * (0.4 if std else 1.0)
        kw = dict(eta_offset=o, sample_weight=w, fit_intercept=fi, rows_per_chunk=RPC,
                  return_sum=True)
        if std:
            kw.update(center=d["center"], scale=d["scale"])
        for kind in ("score", "information"):
            for own in (True, False):
                sel = dict(thetas=coef) if own else dict(beta=coef[1])
                g = M.glm_gram_batched(family, d["X"], y, off, kind=kind, **sel, **kw)
                if kind == "score" and own:
                    g2 = M.glm_gram_batched(family, d["X"], y, off, kind=kind, **sel, **kw)
                    assert all(torch.equal(g[k], g2[k]) for k in g), "two calls differ"
                got = _host(g)
                what = f"{family}-{mask} p={p} ic={int(fi)} std={int(std)} {kind} own={int(own)}"
                _check(got, R.gram_partitions(family, Z, y, off, w=w, o=o, kind=kind, **sel), what)
                _check_sums(got, what)


def test_automatic_chunks(M):
    """rows_per_chunk = 0 (one chunk per partition here) gives the same values
    to the tolerance."""
    d = _dense(33, False)
    g = _host(M.glm_gram_batched("poisson", d["X"], d["poisson"], d["off"], thetas=d["thetas"],
                                 eta_offset=d["o"], sample_weight=d["w"]))
    _check(g, R.gram_partitions("poisson", d["Z"], d["poisson"], d["off"], thetas=d["thetas"],
                                w=d["w"], o=d["o"]), "automatic chunks")


@pytest.mark.parametrize("family", ["logistic", "poisson"])
def test_information_at_the_fit_is_its_sig_inv(M, family):
    """The Gram machinery against the fit's own exact pass: kind="information"
    at fit.theta is fit.sig_inv within 1e-8 of each block's largest entry, the
    fit's parity tolerance (its exact pass may be the int8 one)."""
    d = _dense(13, True, (3001, 1500, 0, 2003))
    y, off = d[family], d["off"]
    if family == "poisson":
        kw = dict(sample_weight=d["w"], eta_offset=d["o"], fit_intercept=True)
        fit = M.poisson_model_batched_weighted(d["X"], y, off, **kw)
    else:
        kw = dict(sample_weight=d["w"], fit_intercept=True)
        fit = M.logistic_model_batched_weighted(d["X"], y, off, **kw)
    assert fit.status.cpu().tolist() == [0, 0, 3, 0]
    g = M.glm_gram_batched(family, d["X"], y, off, thetas=fit.theta, kind="information", **kw)
    a, b = g["gram"].cpu().numpy(), fit.sig_inv.cpu().numpy()
    for k in (0, 1, 3):
        e = float(np.abs(a[k] - b[k]).max() / np.abs(b[k]).max())
        print(f"{family} partition {k}: information vs sig_inv {e:.3e}")
        assert e <= 1e-8, (family, k, e)


# ---- buffers and padded rows: the C entry on a poisoned arena -----------------------------------

@pytest.mark.parametrize("family", ["logistic", "poisson"])
def test_buffers_and_padded_rows(M, family):
    """Inputs and outputs inside a 0xFF-filled arena with guard bands (X at an
    address that is 8 modulo 16), the outputs poisoned: nothing outside the
    outputs is written and no output element is left unwritten.  Then NaN in
    every row of partition 1's y, offset and weight -- partition 0's last block
    holds partition 1's first rows as padding: only partition 1's blocks (and
    the sums) become NaN, every other block keeps its bits.  Then the clean
    inputs over that NaN-laden image of the outputs: the first run's bits."""
    import torch

    from dlsa_amd import _hip

    lib, stream = _hip.load(), torch.cuda.current_stream().cuda_stream
    fam = {"logistic": _hip.FAMILY_LOGISTIC, "poisson": _hip.FAMILY_POISSON}[family]
    d = _dense(15, True)
    has_o = family == "poisson"
    K, P = len(SIZES), 16
    off = d["off"]
    thetas = np.ascontiguousarray(d["thetas"])
    y, o, w = d[family].copy(), d["o"].copy(), d["w"].copy()
    A = PZ.Arena(torch.device("cuda"))
    A.add("X", d["X"].nbytes, 16, 8).add("y", y.nbytes).add("o", o.nbytes).add("w", w.nbytes)
    A.add("thetas", thetas.nbytes)
    outs = (("gram", K * P * P), ("score", K * P), ("gram_sum", P * P), ("score_sum", P))
    for name, n in outs:
        A.add(name, n * 8)
    A.build()
    A.put("X", d["X"])
    A.put("thetas", thetas)

    def run(poison):
        A.put("y", y)
        A.put("o", o)
        A.put("w", w)
        if poison:
            for name, _ in outs:
                A.fill(name, PZ.POISON)
        rc = lib.dlsa_glm_gram_batched_chunked(
            fam, _hip.GRAM_SCORE, A.ptr("X"), A.ptr("y"), A.ptr("o") if has_o else None,
            A.ptr("w"), off.ctypes.data_as(ctypes.c_void_p), K, 15, 1, None, None,
            A.ptr("thetas"), P, RPC, A.ptr("gram"), A.ptr("score"), A.ptr("gram_sum"),
            A.ptr("score_sum"), stream)
        torch.cuda.synchronize()
        _hip.check(rc, "dlsa_glm_gram_batched_chunked")
        A.guards_intact()
        A.inputs_unchanged()
        if poison:
            for name, _ in outs:
                A.fully_written(name, np.float64)
        return dict(gram=A.get("gram", np.float64, (K, P, P)),
                    score=A.get("score", np.float64, (K, P)),
                    gram_sum=A.get("gram_sum", np.float64, (P, P)),
                    score_sum=A.get("score_sum", np.float64))

    clean = run(True)
    _check(clean, R.gram_partitions(family, d["Z"], d[family], off, thetas=thetas, w=d["w"],
                                    o=d["o"] if has_o else None), f"arena {family}")
    _check_sums(clean, f"arena {family}")
    a, b = int(off[1]), int(off[2])
    y[a:b] = o[a:b] = w[a:b] = np.nan
    bad = run(True)
    assert np.isnan(bad["gram"][1]).all() and np.isnan(bad["score"][1]).all()
    assert np.isnan(bad["gram_sum"]).all() and np.isnan(bad["score_sum"]).all()
    for k in (0, 2, 3, 4, 5):
        for name in ("gram", "score"):
            assert PZ.bits_equal(bad[name][k], clean[name][k]), (name, k)
    y[a:b], o[a:b], w[a:b] = d[family][a:b], d["o"][a:b], d["w"][a:b]
    again = run(False)  # over the stale image of the NaN run
    for name in clean:
        assert PZ.bits_equal(again[name], clean[name]), name


def test_error_codes(M):
    """P = 193: DLSA_E_UNSUPPORTED; a stride that is neither 0 nor P and an
    offset with the logistic family: DLSA_E_INVALID -- each before any launch
    (the outputs keep their poison)."""
    import torch

    from dlsa_amd import _hip
    from dlsa_amd._hip import DlsaHipError

    n = 64
    X, y, off = np.zeros((n, 193)), np.zeros(n), np.array([0, n])
    with pytest.raises(DlsaHipError, match=r"\(-3\)"):
        M.glm_gram_batched("logistic", X, y, off, beta=np.zeros(193))
    with pytest.raises(DlsaHipError, match=r"\(-3\)"):
        M.glm_gram_batched("poisson", X[:, :192], y, off, beta=np.zeros(193), fit_intercept=True)
    lib, stream = _hip.load(), torch.cuda.current_stream().cuda_stream
    Xd = torch.zeros((n, 3), dtype=torch.float64, device="cuda")
    v = torch.zeros(n, dtype=torch.float64, device="cuda")
    out = torch.full((16,), float("nan"), dtype=torch.float64, device="cuda")
    offs = np.array([0, n], dtype=np.int64)

    def call(family, o, stride):
        return lib.dlsa_glm_gram_batched(family, 0, Xd.data_ptr(), v.data_ptr(), o, None,
                                         offs.ctypes.data_as(ctypes.c_void_p), 1, 3, 0, None, None,
                                         v.data_ptr(), stride, out.data_ptr(), out.data_ptr(),
                                         None, None, stream)

    assert call(_hip.FAMILY_POISSON, None, 2) == -1
    assert call(_hip.FAMILY_LOGISTIC, v.data_ptr(), 0) == -1
    assert call(1, None, 0) == -3
    torch.cuda.synchronize()
    assert torch.isnan(out).all()


# ---- job level ----------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _job():
    """Over-dispersed counts with exposure and weights: K = 8 partitions (one
    empty), p = 12 and an intercept."""
    sizes = (1500, 1400, 0, 1600, 1300, 1500, 1450, 1550)
    off = _offsets(sizes)
    n, p, r = int(off[-1]), 12, 2.0
    rng = np.random.default_rng(21)
    X = rng.standard_normal((n, p)) * 0.4
    theta = np.concatenate([[0.8], rng.uniform(-0.5, 0.5, p)])
    theta[[3, 6, 7, 10, 11]] = 0.0
    expo = rng.uniform(0.3, 3.0, n)
    mu = expo * np.exp(G.design(X, True) @ theta)
    y = rng.negative_binomial(r, r / (r + mu)).astype(np.float64)
    return X, y, off, expo, G.weights(n, "real")


def _rel(a, b):
    return float(np.abs(np.asarray(a) - np.asarray(b)).max() / np.abs(np.asarray(b)).max())


def test_fit_sharded_cov_types(M):
    """cov_type = "model" / "HC0" / "HC1" on one process against the numpy
    recomputation from the yardstick at the fit's own thetas: cov, std_err and
    wlse within 1e-8, the DBIC support that of finish(info_ref, ...);
    cov_type=None is the call without the keyword."""
    from dlsa_amd.distributed import dlsa_fit_sharded, finish

    X, y, off, expo, w = _job()
    kw = dict(fit_intercept=True, family="poisson", exposure=expo, sample_weight=w)
    plain = dlsa_fit_sharded(X, y, off, **kw)
    none = dlsa_fit_sharded(X, y, off, cov_type=None, **kw)
    assert set(none) == set(plain)
    for key in ("wlse", "oneshot", "beta_byAIC", "beta_byBIC", "dbic_support", "Sig_inv_sum"):
        assert PZ.bits_equal(np.asarray(none[key], np.float64), np.asarray(plain[key], np.float64))
    assert PZ.bits_equal(none["path"]["BIC"], plain["path"]["BIC"])

    fit = plain["fit"]
    P, K = fit.P, fit.K
    th, st = fit.theta.cpu().numpy(), fit.status.cpu().numpy()
    assert st.tolist() == [0, 0, 3, 0, 0, 0, 0, 0]
    ok = st <= 1
    Z, o = G.design(X, True), np.log(expo)
    S = plain["Sig_inv_sum"]
    Mk, _, _ = R.gram_partitions("poisson", Z, y, off, thetas=th, w=w, o=o)
    Mref = Mk[ok].sum(0)
    npos = sum(int((w[a:b] > 0).sum()) for k, (a, b) in enumerate(zip(off[:-1], off[1:])) if ok[k])
    n_all = int(off[-1])

    model = dlsa_fit_sharded(X, y, off, cov_type="model", **kw)
    assert set(model) - set(plain) == {"cov", "std_err", "z", "p_value"}
    assert _rel(model["cov"], np.linalg.inv(S)) <= 1e-8
    assert _rel(model["wlse"], plain["wlse"]) <= 1e-8

    for ct, factor in (("HC0", 1.0), ("HC1", npos / (npos - ok.sum() * P))):
        out = dlsa_fit_sharded(X, y, off, cov_type=ct, **kw)
        assert set(out) - set(plain) == {"cov", "std_err", "z", "p_value", "meat_sum", "info"}
        cov_ref, info_ref = R.sandwich(S, Mref * factor)
        figs = (_rel(out["meat_sum"], Mref), _rel(out["cov"], cov_ref),
                _rel(out["std_err"], np.sqrt(np.diag(cov_ref))), _rel(out["wlse"], plain["wlse"]),
                _rel(out["info"], info_ref))
        print(ct, "meat cov std_err wlse info", " ".join(f"{v:.2e}" for v in figs))
        assert max(figs) <= 1e-8, (ct, figs)
        assert PZ.bits_equal(out["oneshot"], plain["oneshot"])
        assert np.allclose(out["z"], out["wlse"] / out["std_err"], rtol=1e-14, atol=0)
        want = finish(info_ref, info_ref @ plain["wlse"], th[ok].sum(0), float(ok.sum()), n_all,
                      True, "lasso")
        assert out["dbic_support"].tolist() == want["dbic_support"].tolist(), ct
    with pytest.raises(ValueError, match="degrees of freedom"):
        import warnings
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            dlsa_fit_sharded(X[:13], y[:13], [0, 13], cov_type="HC1", fit_intercept=True,
                             family="poisson")


def test_gram_sharded_without_a_group_is_the_local_totals(M):
    from dlsa_amd.distributed import gram_sharded

    d = _dense(15, True)
    kw = dict(thetas=d["thetas"], eta_offset=d["o"], sample_weight=d["w"], fit_intercept=True,
              rows_per_chunk=RPC)
    tot = gram_sharded(d["X"], d["poisson"], d["off"], family="poisson", **kw)
    g = _host(M.glm_gram_batched("poisson", d["X"], d["poisson"], d["off"], return_sum=True, **kw))
    assert PZ.bits_equal(tot["gram_sum"], g["gram_sum"])
    assert PZ.bits_equal(tot["score_sum"], g["score_sum"])


def _rank_worker(rank, world, port, shards, q):
    import torch
    import torch.distributed as dist

    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from dlsa_amd.distributed import gram_sharded

        d = _dense(15, True)
        off = d["off"]
        mine = shards[rank]
        rows = np.concatenate([np.arange(off[k], off[k + 1]) for k in mine])
        offl = np.concatenate([[0], np.cumsum([off[k + 1] - off[k] for k in mine])])
        calls = []
        orig = dist.all_reduce

        def spy(t, *a, **kw):
            calls.append(t.numel())
            return orig(t, *a, **kw)

        dist.all_reduce = spy
        try:
            tot = gram_sharded(d["X"][rows], d["poisson"][rows], offl, thetas=d["thetas"][mine],
                               family="poisson", eta_offset=d["o"][rows],
                               sample_weight=d["w"][rows], fit_intercept=True, rows_per_chunk=RPC)
        finally:
            dist.all_reduce = orig
        q.put((rank, tot["gram_sum"], tot["score_sum"], calls))
    finally:
        dist.destroy_process_group()


def test_gram_sharded_two_ranks_one_gpu(M):
    """Two processes on the one GPU, each with its partitions: ONE all-reduce
    of P^2 + P doubles gives both the single-process totals."""
    import multiprocessing as mp
    import socket

    from dlsa_amd.distributed import gram_sharded

    d = _dense(15, True)
    single = gram_sharded(d["X"], d["poisson"], d["off"], thetas=d["thetas"], family="poisson",
                          eta_offset=d["o"], sample_weight=d["w"], fit_intercept=True,
                          rows_per_chunk=RPC)
    shards = ([0, 2, 4], [1, 3, 5])
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    ctx = mp.get_context("spawn")  # children touch the GPU only after they start
    q = ctx.Queue()
    ps = [ctx.Process(target=_rank_worker, args=(r, 2, port, shards, q)) for r in range(2)]
    for p_ in ps:
        p_.start()
    res = [q.get(timeout=180) for _ in range(2)]
    for p_ in ps:
        p_.join(timeout=60)
        assert p_.exitcode == 0
    P = 16
    _, _, scale = R.gram_partitions("poisson", d["Z"], d["poisson"], d["off"], thetas=d["thetas"],
                                    w=d["w"], o=d["o"])
    for rank, Gt, st, calls in res:
        assert calls == [P * P + P], calls
        # another order of the same six blocks: to the rounding of the sums
        assert _rel(Gt, single["gram_sum"]) <= 1e-13
        assert np.abs(st - single["score_sum"]).max() <= 1e-13 * scale.sum()
    assert PZ.bits_equal(res[0][1], res[1][1]) and PZ.bits_equal(res[0][2], res[1][2])
