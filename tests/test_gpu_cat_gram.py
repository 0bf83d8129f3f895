"""GPU: the score outer-product pass on the categorical-code layout
(``glm_gram_batched_categorical`` / ``dlsa_glm_gram_categorical``) and the
robust covariance on codes (``sandwich_sharded``).

Yardstick: tests/_cat_gram_ref.py -- tests/_gram_ref.py on the dummy-expanded
design, and the a-priori bound of the pass's fixed-point histograms.  Data:
the nine SHAPES of tests/test_gpu_pois_cat.py, built by its functions (three
partitions of 3000-9000 rows plus an empty one): the QN buckets 4 / 8 / 10 /
12 / 16, the exact-bucket (fold) and non-fold kernels, F = 10 (the 16-factor
kernel), no numeric columns, no factors, a one-level factor, standardised
inputs, rows_per_chunk 0 / 1500 / 2000.

Tolerance: tests/test_gpu_gram.py's -- every entry of a partition's ``gram``
within 1e-10 of the yardstick relative to the block's largest entry, ``score``
within 1e-10 of max |Z|^T |s| -- at least four times the a-priori bound of
every case (tests/test_cpu_cat_gram.py checks that condition in numpy).
"""

import ctypes
import functools

import numpy as np
import pytest

import _cat_gram_ref as CR
import _glm_ref as G
import _gram_ref as R
import _poison as PZ
import oracle as O

pytestmark = pytest.mark.gpu

REL = CR.TOL
EMPTY_AT = 1
CASES = [(s, f, m) for s in CR.SHAPES for f, m in CR.FAMILY_MASKS]
CASE_IDS = [f"{CR.SHAPE_IDS[CR.SHAPES.index(s)]}-{f}-{m}" for s, f, m in CASES]


@pytest.fixture(scope="module")
def M():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a visible MI355X"
    from dlsa_amd import models
    return models


def _host(g):
    return {k: v.cpu().numpy() for k, v in g.items()}


def _check(got, want, what, rel=REL):
    """gram per block within rel of its largest entry, score within rel of max
    |Z|^T |s|; exact symmetry; an empty partition all-zero bits.  Prints the
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
    assert worst_g <= rel, (what, "gram", worst_g)
    assert worst_s <= rel, (what, "score", worst_s)


def _check_sums(got, what):
    for name in ("gram", "score"):
        acc = np.zeros(got[name].shape[1:])
        for blk in got[name]:  # k ascending
            acc = acc + blk
        assert PZ.bits_equal(got[name + "_sum"], acc), (what, name + "_sum")


def _call(M, family, d, mask, **kw):
    return M.glm_gram_batched_categorical(family, d["Xn"], d["codes"], d[family], d["off"],
                                          d["levels"], **dict(CR.call_kw(d, mask), **kw))


# ---- 1. the yardstick ------------------------------------------------------------------------

@pytest.mark.parametrize("shape,family,mask", CASES, ids=CASE_IDS)
def test_against_the_yardstick(M, shape, family, mask):
    """Both kinds, at own thetas and at a shared beta; two calls bit-identical;
    the sums over k; the empty partition all-zero bits."""
    import torch

    d = CR.case(shape)
    assert not R.gram_partitions(family, d["Z"], d[family], d["off"], thetas=d["thetas"])[0][
        EMPTY_AT].any()
    for kind in CR.KINDS:
        for own in (True, False):
            sel = dict(thetas=d["thetas"]) if own else dict(beta=d["beta"])
            g = _call(M, family, d, mask, kind=kind, return_sum=True, **sel)
            if own:
                g2 = _call(M, family, d, mask, kind=kind, return_sum=True, **sel)
                assert all(torch.equal(g[k], g2[k]) for k in g), "two calls differ"
            got = _host(g)
            what = f"{family}-{mask} {shape[:2]} {kind} own={int(own)}"
            _check(got, CR.gram(family, d, mask, kind, own), what)
            _check_sums(got, what)


# ---- 2. the dense pass -----------------------------------------------------------------------

@pytest.mark.parametrize("shape", [CR.SHAPES[1], CR.SHAPES[2]],
                         ids=[CR.SHAPE_IDS[1], CR.SHAPE_IDS[2]])
def test_against_the_dense_pass(M, shape):
    """glm_gram_batched on expand_categorical(...): the same tolerance."""
    import torch

    from test_gpu_pois_cat import _ref_kw

    d = CR.case(shape)
    Xd = M.expand_categorical(torch.from_numpy(np.ascontiguousarray(d["Xn"])).cuda(),
                              torch.from_numpy(np.ascontiguousarray(d["codes"])).cuda(),
                              d["levels"])
    for family, mask in (("logistic", "wgt"), ("poisson", "both")):
        o, w = CR.extras(d, mask)
        for kind in CR.KINDS:
            dense = _host(M.glm_gram_batched(family, Xd, d[family], d["off"], thetas=d["thetas"],
                                             kind=kind, eta_offset=o, sample_weight=w,
                                             **_ref_kw(shape)))
            got = _host(_call(M, family, d, mask, kind=kind, thetas=d["thetas"]))
            _, _, scale = CR.gram(family, d, mask, kind, True)
            _check(got, (dense["gram"], dense["score"], scale),
                   f"dense {family}-{mask} {shape[:2]} {kind}")


# ---- 3. information at the fit ---------------------------------------------------------------

@pytest.mark.parametrize("family", ["logistic", "poisson"])
@pytest.mark.parametrize("shape", [CR.SHAPES[1], CR.SHAPES[2], CR.SHAPES[5]],
                         ids=[CR.SHAPE_IDS[i] for i in (1, 2, 5)])
def test_information_at_the_fit_is_its_sig_inv(M, shape, family):
    """kind="information" at fit.theta is fit.sig_inv per entry within 1e-10 of
    sqrt(H_ii H_jj): both sides are fixed-point sums of the same terms, on
    grids that differ."""
    d = CR.case(shape)
    kw = dict(fit_intercept=d["fi"], center=d["center"], scale=d["scale"],
              rows_per_chunk=d["rpc"])
    if family == "poisson":
        ex = dict(sample_weight=d["w"], eta_offset=d["o"])
        fit = M.poisson_model_batched_categorical(d["Xn"], d["codes"], d[family], d["off"],
                                                  d["levels"], tol=1e-12, **ex, **kw)
    else:
        ex = dict(sample_weight=d["w"])
        fit = M.logistic_model_batched_categorical_weighted(
            d["Xn"], d["codes"], d[family], d["off"], d["levels"], tol=1e-12, **ex, **kw)
    assert fit.status.cpu().tolist() == [0, PZ.STATUS_EMPTY, 0, 0]
    g = M.glm_gram_batched_categorical(family, d["Xn"], d["codes"], d[family], d["off"],
                                       d["levels"], thetas=fit.theta, kind="information", **ex,
                                       **kw)
    a, b = g["gram"].cpu().numpy(), fit.sig_inv.cpu().numpy()
    for k in (0, 2, 3):
        dg = np.sqrt(np.abs(np.diag(b[k])))
        e = float((np.abs(a[k] - b[k]) / np.outer(dg, dg)).max())
        print(f"{family} {shape[:2]} partition {k}: information vs sig_inv per entry {e:.3e}")
        assert e <= 1e-10, (family, k, e)
    assert not a[EMPTY_AT].view(np.uint64).any()


# ---- 4. a heavy row --------------------------------------------------------------------------

@pytest.mark.parametrize("family,kind", [("poisson", "score"), ("logistic", "information")])
def test_heavy_row(M, family, kind):
    """One row with omega = 1e4 in partition 2: that partition's gram is within
    the a-priori bound computed for it (plus 1e-13 of the largest entry), and
    the other partitions keep the bits of the call without the heavy row."""
    shape = CR.SHAPES[2]
    d = CR.case(shape)
    mask = "both" if family == "poisson" else "wgt"
    o, _ = CR.extras(d, mask)
    off = d["off"]
    w = d["w"].copy()
    row = int(off[2]) + 17
    w[row] = 1e4
    base = _host(_call(M, family, d, mask, kind=kind, thetas=d["thetas"]))
    got = _host(_call(M, family, d, mask, kind=kind, thetas=d["thetas"], sample_weight=w))
    for k in (0, 1, 3):
        for name in ("gram", "score"):
            assert PZ.bits_equal(got[name][k], base[name][k]), (name, k)
    Gw, sw, scale = R.gram_partitions(family, d["Z"], d[family], off, thetas=d["thetas"], w=w,
                                      o=o, kind=kind)
    bg, bs = CR.bound(family, d["Z"], d[family], off, d["thetas"], d["q"], d["fi"], d["rpc"],
                      w=w, o=o, kind=kind)
    eg = float(np.abs(got["gram"][2] - Gw[2]).max() / np.abs(Gw[2]).max())
    es = float(np.abs(got["score"][2] - sw[2]).max() / scale[2])
    print(f"heavy row {family} {kind}: gram {eg:.3e} (bound {bg[2]:.3e}) "
          f"score {es:.3e} (bound {bs[2]:.3e})")
    assert eg <= bg[2] + 1e-13, (eg, bg[2])
    assert es <= bs[2] + 1e-13, (es, bs[2])
    assert np.array_equal(got["gram"][2], got["gram"][2].T)


# ---- 5, 6. the C entry on a poisoned arena ---------------------------------------------------

class _Abi:
    """The inputs and outputs of one shape inside a 0xFF-filled arena with
    guard bands; run() poisons the outputs, calls the entry and checks the
    guards, the inputs and (on success) that every output element was
    written."""

    def __init__(self, shape, family):
        import torch

        from dlsa_amd import _hip

        self.hip, self.lib = _hip, _hip.load()
        self.stream = torch.cuda.current_stream().cuda_stream
        self.torch = torch
        d = self.d = CR.case(shape)
        self.family = family
        self.fam = {"logistic": _hip.FAMILY_LOGISTIC, "poisson": _hip.FAMILY_POISSON}[family]
        self.K, self.P = d["K"], d["P"]
        self.y, self.o, self.w = d[family].copy(), d["o"].copy(), d["w"].copy()
        self.codes = np.ascontiguousarray(d["codes"]).copy()
        self.thetas = np.ascontiguousarray(d["thetas"])
        self.lv = np.asarray(d["levels"], dtype=np.int32)
        A = self.A = PZ.Arena(torch.device("cuda"))
        A.add("Xn", d["Xn"].nbytes, 16, 8).add("codes", self.codes.nbytes, 16, 3)
        A.add("y", self.y.nbytes).add("o", self.o.nbytes).add("w", self.w.nbytes)
        A.add("thetas", self.thetas.nbytes)
        K, P = self.K, self.P
        self.outs = (("gram", K * P * P), ("score", K * P), ("gram_sum", P * P),
                     ("score_sum", P))
        for name, n in self.outs:
            A.add(name, n * 8)
        A.build()
        A.put("Xn", np.ascontiguousarray(d["Xn"]))
        A.put("thetas", self.thetas)

    def run(self, kind=0, with_o=None, stride=None, poison=True):
        A, d = self.A, self.d
        A.put("codes", self.codes)
        A.put("y", self.y)
        A.put("o", self.o)
        A.put("w", self.w)
        if poison:
            for name, _ in self.outs:
                A.fill(name, PZ.POISON)
        with_o = self.family == "poisson" if with_o is None else with_o
        rc = self.lib.dlsa_glm_gram_categorical(
            self.fam, kind, A.ptr("Xn") if d["q"] else None,
            A.ptr("codes") if len(self.lv) else None, A.ptr("y"),
            A.ptr("o") if with_o else None, A.ptr("w"),
            d["off"].ctypes.data_as(ctypes.c_void_p), self.K, d["q"], len(self.lv),
            self.lv.ctypes.data_as(ctypes.c_void_p), int(d["fi"]), None, None, A.ptr("thetas"),
            self.P if stride is None else stride, d["rpc"], A.ptr("gram"), A.ptr("score"),
            A.ptr("gram_sum"), A.ptr("score_sum"), self.stream)
        self.torch.cuda.synchronize()
        A.guards_intact()
        A.inputs_unchanged()
        if rc == 0 and poison:
            for name, _ in self.outs:
                A.fully_written(name, np.float64)
        K, P = self.K, self.P
        return rc, dict(gram=A.get("gram", np.float64, (K, P, P)),
                        score=A.get("score", np.float64, (K, P)),
                        gram_sum=A.get("gram_sum", np.float64, (P, P)),
                        score_sum=A.get("score_sum", np.float64))

    def untouched(self):
        """Every output byte still holds the poison."""
        for name, _ in self.outs:
            assert (self.A.get(name, np.uint8) == PZ.POISON).all(), name


@pytest.mark.parametrize("family", ["logistic", "poisson"])
def test_nan_weight_and_offset_stay_in_their_partition(M, family):
    """The clean call on the arena against the yardstick; then a NaN weight
    (Poisson: and a NaN offset on another row) in partition 2: its gram and
    score are all NaN, every other partition keeps the clean call's bits; then
    the clean inputs over the NaN-laden outputs: the first run's bits."""
    shape = CR.SHAPES[5]  # (not standardised: the arena call passes no center / scale)
    t = _Abi(shape, family)
    d, off = t.d, t.d["off"]
    mask = "both" if family == "poisson" else "wgt"
    rc, clean = t.run()
    t.hip.check(rc, "dlsa_glm_gram_categorical")
    _check(clean, CR.gram(family, d, mask, "score", True), f"arena {family}")
    _check_sums(clean, f"arena {family}")
    a = int(off[2])
    t.w[a + 5] = np.nan
    if family == "poisson":
        t.o[a + 1200] = np.nan
    rc, bad = t.run()
    t.hip.check(rc, "dlsa_glm_gram_categorical")
    assert np.isnan(bad["gram"][2]).all() and np.isnan(bad["score"][2]).all()
    assert np.isnan(bad["gram_sum"]).all() and np.isnan(bad["score_sum"]).all()
    for k in (0, 1, 3):
        for name in ("gram", "score"):
            assert PZ.bits_equal(bad[name][k], clean[name][k]), (name, k)
    t.w[a + 5], t.o[a + 1200] = d["w"][a + 5], d["o"][a + 1200]
    rc, again = t.run(poison=False)  # over the stale image of the NaN run
    assert rc == 0
    for name in clean:
        assert PZ.bits_equal(again[name], clean[name]), name


def test_error_codes(M):
    """A code >= levels[f], an offset with the logistic family, a bad kind and
    a bad stride give DLSA_E_INVALID through the C ABI and leave the poisoned
    outputs alone.  No layout within the entry's shape limits (P <= 192,
    intercept + q <= 16, F <= 16) overflows the LDS -- the largest histograms,
    16 factors of 12 levels beside 16 numeric columns, stay under 160 KiB with
    one replica each -- so that error cannot be provoked: the largest layout is
    accepted instead."""
    from dlsa_amd import _hip

    t = _Abi(CR.SHAPES[0], "logistic")
    rc, _ = t.run(with_o=True)
    assert rc == -1 and "Poisson" in _hip.last_error()
    t.untouched()
    rc, _ = t.run(kind=2)
    assert rc == -1
    t.untouched()
    rc, _ = t.run(stride=3)
    assert rc == -1 and "stride" in _hip.last_error()
    t.untouched()
    row = int(t.d["off"][3]) + 11
    t.codes[row, 1] = t.lv[1]  # the first invalid code of factor 1
    rc, _ = t.run()
    assert rc == -1 and "partition 3: 1 level codes" in _hip.last_error()
    t.untouched()
    t.codes[row, 1] = 0
    rc, _ = t.run()
    assert rc == 0

    import torch

    lv = np.full(16, 12, dtype=np.int32)
    P = 16 + 16 * 11
    offs = np.array([0, 0], dtype=np.int64)
    out = torch.full((P * P + P,), float("nan"), dtype=torch.float64, device="cuda")
    beta = torch.zeros(P, dtype=torch.float64, device="cuda")
    rc = _hip.load().dlsa_glm_gram_categorical(
        _hip.FAMILY_LOGISTIC, 0, None, None, None, None, None,
        offs.ctypes.data_as(ctypes.c_void_p), 1, 16, 16, lv.ctypes.data_as(ctypes.c_void_p), 0,
        None, None, beta.data_ptr(), 0, 0, out.data_ptr(), out[P * P:].data_ptr(), None, None,
        torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert rc == 0, _hip.last_error()
    assert not out.cpu().numpy().view(np.uint64).any()  # the empty partition: exact zeros


# ---- 7. sandwich_sharded on codes -----------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _job(family):
    """K = 8 partitions (one empty) on codes: 4 numeric columns, factors of 4,
    3 and 5 levels, an intercept; over-dispersed counts with exposure and
    weights (Poisson) or 0/1 responses (logistic)."""
    sizes = (1500, 1400, 0, 1600, 1300, 1500, 1450, 1550)
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    n, q, levels, r = int(off[-1]), 4, [4, 3, 5], 2.0
    rng = np.random.default_rng(31)
    Xn = rng.standard_normal((n, q)) * 0.4
    codes = np.stack([rng.integers(0, L, n) for L in levels], 1).astype(np.uint8)
    Z = G.design(O.expand_codes(Xn, codes, levels), True)
    theta = np.concatenate([[0.5], rng.uniform(-0.5, 0.5, Z.shape[1] - 1)])
    theta[[2, 6, 9]] = 0.0
    expo = rng.uniform(0.3, 3.0, n)
    if family == "poisson":
        mu = expo * np.exp(Z @ theta)
        y = rng.negative_binomial(r, r / (r + mu)).astype(np.float64)
        kw = dict(exposure=expo, sample_weight=G.weights(n, "real"))
    else:
        y = (rng.uniform(size=n) < G._expit(Z @ theta)).astype(np.float64)
        kw = {}
    return Xn, codes, levels, y, off, Z, kw


def _rel(a, b):
    return float(np.abs(np.asarray(a) - np.asarray(b)).max() / np.abs(np.asarray(b)).max())


@pytest.mark.parametrize("family", ["logistic", "poisson"])
def test_sandwich_sharded_on_codes(M, family):
    """cov, info and std_err within 1e-8 of the numpy recomputation from the
    yardstick at the returned fit.theta, the DBIC support that of
    finish(info_ref, ...), HC1 = HC0 x n+ / (n+ - K_ok P); dlsa_fit_sharded
    itself still refuses cov_type with codes."""
    from dlsa_amd.distributed import dlsa_fit_sharded, finish, sandwich_sharded

    Xn, codes, levels, y, off, Z, ex = _job(family)
    kw = dict(fit_intercept=True, family=family, codes=codes, levels=levels, **ex)
    with pytest.raises(ValueError, match="dense layout only"):
        dlsa_fit_sharded(Xn, y, off, cov_type="HC0", **kw)
    plain = dlsa_fit_sharded(Xn, y, off, **kw)
    fit = plain["fit"]
    P = fit.P
    th, st = fit.theta.cpu().numpy(), fit.status.cpu().numpy()
    assert st.tolist() == [0, 0, 3, 0, 0, 0, 0, 0]
    ok = st <= 1
    w = ex.get("sample_weight")
    o = np.log(ex["exposure"]) if "exposure" in ex else None
    S = plain["Sig_inv_sum"]
    Mk, _, _ = R.gram_partitions(family, Z, y, off, thetas=th, w=w, o=o)
    Mref = Mk[ok].sum(0)
    ww = np.ones(len(y)) if w is None else w
    npos = sum(int((ww[a:b] > 0).sum()) for k, (a, b) in enumerate(zip(off[:-1], off[1:]))
               if ok[k])
    hc = {}
    for ct, factor in (("HC0", 1.0), ("HC1", npos / (npos - ok.sum() * P))):
        out = hc[ct] = sandwich_sharded(fit, Xn, y, off, cov_type=ct, **kw)
        assert set(out) | {"fit"} == set(plain) | {"cov", "std_err", "z", "p_value", "meat_sum",
                                                   "info"}
        cov_ref, info_ref = R.sandwich(S, Mref * factor)
        figs = (_rel(out["meat_sum"], Mref), _rel(out["cov"], cov_ref),
                _rel(out["std_err"], np.sqrt(np.diag(cov_ref))), _rel(out["wlse"], plain["wlse"]),
                _rel(out["info"], info_ref))
        print(family, ct, "meat cov std_err wlse info", " ".join(f"{v:.2e}" for v in figs))
        assert max(figs) <= 1e-8, (ct, figs)
        assert PZ.bits_equal(out["oneshot"], plain["oneshot"])
        want = finish(info_ref, info_ref @ plain["wlse"], th[ok].sum(0), float(ok.sum()),
                      int(off[-1]), True, "lasso")
        assert out["dbic_support"].tolist() == want["dbic_support"].tolist(), ct
    f1 = npos / (npos - ok.sum() * P)
    # (two solves with A = sum Sig_inv each: a few cond(A) eps of the largest entry)
    e1 = _rel(hc["HC1"]["cov"], hc["HC0"]["cov"] * f1)
    print(family, f"HC1 vs HC0 x n+ / (n+ - K_ok P): {e1:.2e}")
    assert e1 <= 1e-10, e1
    with pytest.raises(ValueError, match="HC3"):
        sandwich_sharded(fit, Xn, y, off, cov_type="HC3", **kw)


def test_sandwich_sharded_dense_is_dlsa_fit_sharded(M):
    """On the dense layout sandwich_sharded(out["fit"], X, ...) gives the bits
    of dlsa_fit_sharded(X, ..., cov_type=...) in one process."""
    from dlsa_amd.distributed import dlsa_fit_sharded, sandwich_sharded

    Xn, codes, levels, y, off, Z, ex = _job("poisson")
    X = np.ascontiguousarray(Z[:, 1:])
    kw = dict(fit_intercept=True, family="poisson", **ex)
    for ct in ("HC0", "HC1", "HC3"):
        out = dlsa_fit_sharded(X, y, off, cov_type=ct, **kw)
        again = sandwich_sharded(out["fit"], X, y, off, cov_type=ct, **kw)
        for key in ("cov", "std_err", "info", "meat_sum", "wlse", "z", "p_value", "beta_byBIC"):
            assert PZ.bits_equal(np.asarray(again[key], np.float64),
                                 np.asarray(out[key], np.float64)), (ct, key)
        assert again["dbic_support"].tolist() == out["dbic_support"].tolist()


def test_gram_sharded_on_codes_is_the_local_totals(M):
    from dlsa_amd.distributed import gram_sharded

    d = CR.case(CR.SHAPES[1])
    kw = CR.call_kw(d, "both")
    tot = gram_sharded(d["Xn"], d["poisson"], d["off"], thetas=d["thetas"], family="poisson",
                       codes=d["codes"], levels=d["levels"], **kw)
    g = _host(_call(M, "poisson", d, "both", thetas=d["thetas"], return_sum=True))
    assert PZ.bits_equal(tot["gram_sum"], g["gram_sum"])
    assert PZ.bits_equal(tot["score_sum"], g["score_sum"])
