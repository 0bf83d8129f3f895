"""Per-row prior weights on the GPU: the weighted logistic and Poisson fits
(dlsa_*_fit_batched_weighted through the ``*_weighted`` functions of
dlsa_amd.models) and the weighted evaluation pass.

Yardsticks: the library's own unweighted fit of the row-replicated data (both
sides on the GPU) and the numpy fp64 Newton of tests/_glm_ref.py.
Tolerances are the project's contracts: theta and Sig_inv theta within 1e-8
relative to the largest entry, Sig_inv per entry |d_ij| / sqrt(H_ii H_jj) <
1e-10, the log-likelihood within 1e-9 relative; statuses equal.

Shapes are the suite's smallest that cross every structural edge: P = 13 / 14
(NT = 1), P = 100 / 101 (NT = 7: two per-wave waves and the edge strip), P =
129 (the cooperative fp64 exact pass, 8 waves), partition sizes that are no
multiple of 32 with an empty partition, and 1024-row chunks so partitions
span several chunks with tail blocks.

The fits run with tol = 1e-12, not the default 1e-10: Sig_inv is published by
the pass at the iterate BEFORE the last Newton step, whose size is what tol
bounds (max|step| <= tol (1 + max|theta|)), so at the default each fit's
Sig_inv may lie 1e-10 (relative, per entry) from the Hessian at its theta --
the whole of the per-entry contract, before two such fits are compared with
each other.  With a last step below 1e-12 that share is 1e-12.
"""

import ctypes
import functools

import numpy as np
import pytest

import _glm_ref as G
import oracle as O
from _poison import FUSED_SIZES, FUSED_SIZES_BIG, STATUS_EMPTY, STATUS_NONFINITE, \
    STATUS_SINGULAR, bits_equal

pytestmark = pytest.mark.gpu

REL = 1e-8
REL_S = 1e-10
REL_LL = 1e-9
TOL = 1e-12  # of the fits (the module docstring)
RPC = 1024
FIELDS = ("theta", "sig_inv", "sig_inv_theta", "loglik", "iters", "status")


@pytest.fixture(scope="module")
def M():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a visible MI355X"
    from dlsa_amd import models
    return models


def _rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)


def _per_entry(S, H):
    d = np.sqrt(np.abs(np.diag(H)))
    return (np.abs(S - H) / np.outer(d, d)).max()


def _sizes(p, fi):
    return FUSED_SIZES if p + fi <= 128 else FUSED_SIZES_BIG


def _host(fit):
    return {f: getattr(fit, f).cpu().numpy() for f in FIELDS}


@functools.lru_cache(maxsize=None)
def _data(family, p, fi):
    """(X, y, o or None, offsets) of one shape; family is logistic, poisson,
    poisson_offset or binomial (then y = s / m and the trial counts m ride in
    the third slot)."""
    sizes = _sizes(p, fi)
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    n = int(off[-1])
    if family in ("logistic", "binomial"):
        X, y = O.simulate_counter(n, p, seed=100 + p)
        X = np.ascontiguousarray(X)
        if family == "logistic":
            return X, y, None, off
        rng = np.random.default_rng(p)
        m = rng.integers(1, 5, n)
        b = np.zeros(p)
        b[:max(1, int(0.4 * p))] = 1.0
        s = rng.binomial(m, 1.0 / (1.0 + np.exp(-(X @ b + (0.3 if fi else 0.0)))))
        return X, s.astype(np.float64), m.astype(np.float64), off
    X, y, o = G.simulate_offset(n, p, fit_intercept=fi)
    if family == "poisson":
        b = np.zeros(p)
        b[:max(1, int(0.4 * p))] = 0.5
        y = np.random.default_rng(7).poisson(np.exp(X @ b + (1.0 if fi else 0.0))).astype(float)
        o = None
    return X, y, o, off


def _fit(M, family, X, y, o, off, fi, hessian, w=None, **kw):
    """w None: the unweighted entry as it stands; else the weighted one."""
    kw = dict(fit_intercept=fi, hessian=hessian, rows_per_chunk=RPC, tol=TOL, **kw)
    logistic = family in ("logistic", "binomial")
    if w is not None:
        if logistic:
            return M.logistic_model_batched_weighted(X, y, off, sample_weight=w, **kw)
        return M.poisson_model_batched_weighted(X, y, off, sample_weight=w, eta_offset=o, **kw)
    if logistic:
        return M.logistic_model_batched(X, y, off, **kw)
    if o is None:
        return M.poisson_model_batched(X, y, off, **kw)
    return M.poisson_model_batched_offset(X, y, off, eta_offset=o, **kw)


def _compare(got, want, tag, iters_pm1=False):
    """got against want (host dicts of the fit fields) at the contracts."""
    assert got["status"].tolist() == want["status"].tolist(), (tag, got["status"], want["status"])
    for k, st in enumerate(want["status"]):
        if st != 0:
            continue
        e = (_rel(got["theta"][k], want["theta"][k]),
             _per_entry(got["sig_inv"][k], want["sig_inv"][k]),
             _rel(got["sig_inv_theta"][k], want["sig_inv_theta"][k]),
             abs(got["loglik"][k] - want["loglik"][k]) / abs(want["loglik"][k]))
        print(f"{tag} k={k} theta {e[0]:.2e} sig_inv/entry {e[1]:.2e} sig_inv_theta {e[2]:.2e} "
              f"loglik {e[3]:.2e} iters {int(got['iters'][k])} vs {int(want['iters'][k])}")
        assert e[0] < REL and e[1] < REL_S and e[2] < REL and e[3] < REL_LL, (tag, k, e)
        if iters_pm1:
            assert abs(int(got["iters"][k]) - int(want["iters"][k])) <= 1, \
                (tag, k, int(got["iters"][k]), int(want["iters"][k]))


# ---- 1. replication, against the code as it stands --------------------------------

REPLICATION = [
    ("logistic", 13, False, "mixed", "int"), ("logistic", 13, True, "mixed", "spread"),
    ("logistic", 13, True, "mixed_f32", "int"), ("logistic", 100, True, "mixed", "int"),
    ("logistic", 100, False, "fp64", "int"), ("logistic", 129, False, "mixed", "int"),
    ("poisson", 13, True, "mixed", "int"), ("poisson", 100, False, "mixed", "spread"),
    ("poisson", 129, False, "fp64", "int"),
    ("poisson_offset", 13, False, "mixed", "int"), ("poisson_offset", 100, True, "mixed", "int"),
    ("poisson_offset", 100, True, "mixed_f32", "int"), ("poisson_offset", 129, False, "mixed", "int"),
]


@pytest.mark.parametrize("family,p,fi,hessian,kind", REPLICATION)
def test_replication(M, family, p, fi, hessian, kind):
    """omega in {0, 1, 2, 3} (or {0, 1, 50}): the weighted fit of the n rows
    against the unweighted entry on the replicated rows, rows with omega = 0
    left out.  In mixed mode iters agree within one: an omega missing from
    the bf16 image would still converge through the exact gradient, but later."""
    X, y, o, off = _data(family, p, fi)
    w = G.weights(len(y), kind)
    got = _host(_fit(M, family, X, y, o, off, fi, hessian, w=w))
    arrays = (X, y) if o is None else (X, y, o)
    rep = G.replicate(w, *arrays)
    roff = G.replicate_offsets(w, off)
    want = _host(_fit(M, family, rep[0], rep[1], None if o is None else rep[2], roff, fi, hessian))
    assert want["status"].tolist() == [0, STATUS_EMPTY, 0, 0, 0]
    _compare(got, want, f"rep {family} p={p} fi={fi} {hessian} {kind}", iters_pm1=hessian == "mixed")


@pytest.mark.parametrize("p,fi", [(13, True), (100, False)])
def test_grouped_binomial(M, p, fi):
    """y = s / m with omega = m against the expanded 0/1 rows."""
    X, s, m, off = _data("binomial", p, fi)
    got = _host(_fit(M, "logistic", X, s / m, None, off, fi, "mixed", w=m))
    Xe, ye, offe = G.expand_binomial(X, s, m, off)
    want = _host(_fit(M, "logistic", Xe, ye, None, offe, fi, "mixed"))
    _compare(got, want, f"binomial p={p} fi={fi}", iters_pm1=True)


# ---- 2. real-valued omega against the numpy reference -----------------------------

REAL = [
    ("logistic", 13, False, "mixed", False), ("logistic", 100, True, "mixed", False),
    ("logistic", 129, False, "fp64", False), ("logistic", 13, True, "mixed_f32", True),
    ("poisson", 13, True, "fp64", False), ("poisson", 100, False, "mixed", False),
    ("poisson_offset", 100, True, "mixed", False), ("poisson_offset", 129, False, "mixed", False),
    ("poisson_offset", 13, True, "mixed", True),
]


@pytest.mark.parametrize("family,p,fi,hessian,std", REAL)
def test_real_weights(M, family, p, fi, hessian, std):
    X, y, o, off = _data(family, p, fi)
    w = G.weights(len(y), "real")
    kw = {}
    if std:  # columns worth standardising
        X = X * np.linspace(0.5, 3.0, p) + np.linspace(-1.0, 2.0, p)
        kw = dict(center=X.mean(0), scale=X.std(0, ddof=1))
        if family != "logistic":
            y = np.random.default_rng(3).poisson(np.exp(
                0.5 + 0.3 * ((X - kw["center"]) / kw["scale"])[:, :4].sum(1)
                + (0.0 if o is None else o))).astype(float)
    fam = "logistic" if family == "logistic" else "poisson"
    ref = G.fit_partitions(fam, X, y, off, w=w, o=o, fit_intercept=fi, **kw)
    fit = _fit(M, family, X, y, o, off, fi, hessian, w=w, **kw)
    got = _host(fit)
    assert got["status"].tolist() == [0, STATUS_EMPTY, 0, 0, 0]
    ref["status"] = got["status"]
    _compare(got, ref, f"real {family} p={p} fi={fi} {hessian} std={std}")
    assert fit.stats["passes_oz"] == 0


# ---- 3. omega = 1, None and NULL ---------------------------------------------------

def _abi_fit(M, entry, X, y, off, fi, extra, hessian="fp64"):
    """A fit entry through ctypes directly: `extra` are the pointers between y
    and offsets (None: NULL)."""
    import torch

    from dlsa_amd import _hip

    dev = torch.device("cuda")
    Xd = torch.from_numpy(X).to(dev)
    yd = torch.from_numpy(y).to(dev)
    K, p = len(off) - 1, X.shape[1]
    P = p + int(fi)
    outs = [torch.full(s, 7.0, dtype=torch.float64, device=dev)
            for s in ((K, P), (K, P, P), (K, P), (K,))]
    outs += [torch.full((K,), 7, dtype=torch.int32, device=dev) for _ in range(2)]
    opt = _hip.default_options()
    opt.hessian_mode = {"mixed": _hip.HESSIAN_MIXED, "fp64": _hip.HESSIAN_FP64}[hessian]
    opt.rows_per_chunk = RPC
    offs = np.ascontiguousarray(off, dtype=np.int64)
    ptr = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())  # noqa: E731
    rc = getattr(_hip.load(), entry)(
        ptr(Xd), ptr(yd), *[ptr(e) for e in extra], offs.ctypes.data_as(ctypes.c_void_p), K, p,
        int(fi), None, None, 100, TOL, *[ptr(t) for t in outs], ctypes.byref(opt),
        ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
    torch.cuda.synchronize()
    return rc, dict(zip(FIELDS, [t.cpu().numpy() for t in outs]))


@pytest.mark.parametrize("family", ["logistic", "poisson", "poisson_offset"])
def test_unit_weights_none_and_null(M, family):
    import torch

    p, fi = 100, True
    X, y, o, off = _data(family, p, fi)
    base = _fit(M, family, X, y, o, off, fi, "fp64")
    ones = _fit(M, family, X, y, o, off, fi, "fp64", w=np.ones(len(y)))
    hb, ho = _host(base), _host(ones)
    assert hb["status"].tolist() == ho["status"].tolist() == [0, STATUS_EMPTY, 0, 0, 0]
    for k in (0, 2, 3, 4):
        e = [_rel(ho[f][k], hb[f][k]) for f in ("theta", "sig_inv", "sig_inv_theta", "loglik")]
        print(f"{family} unit weights k={k}", " ".join(f"{v:.2e}" for v in e))
        assert max(e) < 1e-12
    print(f"{family} unit weights bitwise equal:", {f: bits_equal(ho[f], hb[f]) for f in FIELDS})
    # None is today's call; a NULL pointer into the weighted entry too, bit for bit
    none = (M.logistic_model_batched_weighted(X, y, off, sample_weight=None, fit_intercept=fi,
                                              rows_per_chunk=RPC) if family == "logistic" else
            M.poisson_model_batched_weighted(X, y, off, sample_weight=None, eta_offset=o,
                                             fit_intercept=fi, rows_per_chunk=RPC))
    plain = (M.logistic_model_batched(X, y, off, fit_intercept=fi, rows_per_chunk=RPC)
             if family == "logistic" else
             M.poisson_model_batched(X, y, off, fit_intercept=fi, rows_per_chunk=RPC)
             if o is None else
             M.poisson_model_batched_offset(X, y, off, eta_offset=o, fit_intercept=fi,
                                            rows_per_chunk=RPC))
    for f in FIELDS:
        assert torch.equal(getattr(none, f), getattr(plain, f)), f
    od = None if o is None else torch.from_numpy(o).cuda()
    if family == "logistic":
        rc, null = _abi_fit(M, "dlsa_logistic_fit_batched_weighted", X, y, off, fi, [None])
    else:
        rc, null = _abi_fit(M, "dlsa_poisson_fit_batched_weighted", X, y, off, fi, [od, None])
    assert rc == 0
    for f in FIELDS:
        assert bits_equal(null[f], hb[f]), f


# ---- 4. bad weights ------------------------------------------------------------------

BAD_SIZES = (1500, 2000, 2003)


@pytest.mark.parametrize("hessian", ["mixed", "fp64"])
@pytest.mark.parametrize("family", ["logistic", "poisson_offset", "poisson"])
@pytest.mark.parametrize("bad,where", [(np.nan, "first"), (np.inf, "middle"), (-1.0, "last")])
def test_bad_weight(M, family, bad, where, hessian):
    """The bad weight ends its partition NONFINITE with all-zero outputs; the
    others are the run without it, bit for bit.  "first": the first row of
    partition 1, which the last block of partition 0 (1500 rows: 28 of a
    32-row block, 12 of a 16-row one) reads as a padded row."""
    p, fi = 8, True
    off = np.concatenate([[0], np.cumsum(BAD_SIZES)]).astype(np.int64)
    n = int(off[-1])
    if family == "logistic":
        X, y = O.simulate_counter(n, p, seed=5)
        o = None
    elif family == "poisson":  # the weighted kernels without the offset stream
        X, y = G.simulate(n, p, seed=7, fit_intercept=fi)
        o = None
    else:
        X, y, o = G.simulate_offset(n, p, fit_intercept=fi)
    import torch

    w = G.weights(n, "real").copy()
    wb = w.copy()
    wb[{"first": off[1], "middle": (off[1] + off[2]) // 2, "last": off[2] - 1}[where]] = bad
    with pytest.raises(ValueError, match="sample_weight"):  # the Python layer refuses it
        _fit(M, family, X, y, o, off, fi, hessian, w=wb)

    def run(wv):  # so the library's own check is reached through the C-ABI
        wd = torch.from_numpy(wv).cuda()
        if family == "logistic":
            return _abi_fit(M, "dlsa_logistic_fit_batched_weighted", X, y, off, fi, [wd], hessian)
        return _abi_fit(M, "dlsa_poisson_fit_batched_weighted", X, y, off, fi,
                        [None if o is None else torch.from_numpy(o).cuda(), wd], hessian)

    rc, clean = run(w)
    assert rc == 0 and clean["status"].tolist() == [0, 0, 0]
    rc, got = run(wb)
    assert rc == 0 and got["status"].tolist() == [0, STATUS_NONFINITE, 0]
    for f in FIELDS:
        assert bits_equal(got[f][[0, 2]], clean[f][[0, 2]]), f
    for f in ("theta", "sig_inv", "sig_inv_theta", "loglik", "iters"):
        assert not got[f][1].any(), f


@pytest.mark.parametrize("family", ["logistic", "poisson"])
def test_zero_weight_partition_is_singular(M, family):
    p, fi = 8, True
    off = np.concatenate([[0], np.cumsum(BAD_SIZES)]).astype(np.int64)
    n = int(off[-1])
    if family == "logistic":
        X, y = O.simulate_counter(n, p, seed=5)
    else:
        X, y, _ = G.simulate_offset(n, p, fit_intercept=fi)
    w = G.weights(n, "real").copy()
    clean = _host(_fit(M, family, X, y, None, off, fi, "mixed", w=w))
    w[off[1]:off[2]] = 0.0
    got = _host(_fit(M, family, X, y, None, off, fi, "mixed", w=w))
    assert got["status"].tolist() == [0, STATUS_SINGULAR, 0]
    for f in FIELDS:
        assert bits_equal(got[f][[0, 2]], clean[f][[0, 2]]), f
    for f in ("theta", "sig_inv", "sig_inv_theta", "loglik", "iters"):
        assert not got[f][1].any(), f


# ---- 5. evaluation ----------------------------------------------------------------------

@pytest.mark.parametrize("family,p", [("logistic", 13), ("logistic", 100), ("poisson", 13),
                                      ("poisson_offset", 13), ("poisson_offset", 100)])
def test_evaluation(M, family, p):
    """B = 3 candidates (the weighted fit's theta of partition 0, 0.9 of it,
    zeros) per partition and summed, against numpy to 1e-12 relative."""
    fi = True
    X, y, o, off = _data(family, p, fi)
    w = G.weights(len(y), "real")
    fit = _fit(M, family, X, y, o, off, fi, "mixed", w=w)
    th = fit.theta[0].cpu().numpy()
    betas = np.stack([th, 0.9 * th, np.zeros(p + 1)])
    Z = G.design(X, fi)
    parts = [k for k in range(len(off) - 1) if off[k + 1] > off[k]]

    def ll(a, b, bt):
        if family == "logistic":
            return G.loglik("logistic", Z[a:b], y[a:b], bt, w[a:b])
        return G.loglik("poisson", Z[a:b], y[a:b], bt, w[a:b], None if o is None else o[a:b])

    want = np.array([[ll(off[k], off[k + 1], bt) for bt in betas] for k in parts])
    kw = dict(fit_intercept=fi, return_sum=True, sample_weight=w)
    if family == "logistic":
        got, tot = M.logistic_loglik_batched(X, y, off, betas, **kw)
    else:
        got, tot = M.poisson_loglik_batched_weighted(X, y, off, betas, eta_offset=o, **kw)
    got, tot = got.cpu().numpy(), tot.cpu().numpy()
    assert got.shape == (len(off) - 1, 3) and tot.shape == (3,)
    assert not got[1].any()  # the empty partition
    e = (np.abs(got[parts] / want - 1).max(), np.abs(tot / want.sum(0) - 1).max())
    print(f"eval {family} p={p}: per partition {e[0]:.2e} summed {e[1]:.2e}")
    assert e[0] < 1e-12 and e[1] < 1e-12
    # the fit's loglik is the weighted evaluation at its theta
    fitted = float(fit.loglik[0])
    assert abs(got[0, 0] - fitted) < REL_LL * abs(fitted)


# ---- 6. workspace hygiene -------------------------------------------------------------

@pytest.mark.parametrize("family", ["logistic", "poisson", "poisson_offset"])
def test_workspace_hygiene(M, family):
    """A zero-filled, a 0xFF-filled and a stale workspace (left by a fit of the
    other family with more partitions): bit-identical outputs."""
    import torch

    from dlsa_amd import _hip

    p, fi = 100, True
    X, y, o, off = _data(family, p, fi)
    w = G.weights(len(y), "real")
    other = "poisson" if family == "logistic" else "logistic"
    Xs, ys, _, offs = _data(other, 129, False)
    lib = _hip.load()
    need = max(lib.dlsa_logistic_workspace_bytes(o_.ctypes.data_as(ctypes.c_void_p), len(o_) - 1,
                                                 p_, f_, RPC)
               for o_, p_, f_ in ((off, p, 1), (offs, 129, 0)))
    runs = {}
    for kind in ("zero", "ff", "stale"):
        ws = torch.full((need,), 0xFF if kind == "ff" else 0, dtype=torch.uint8, device="cuda")
        if kind == "stale":
            _fit(M, other, Xs, ys, None, offs, False, "mixed", max_iter=2, workspace=ws)
        runs[kind] = _host(_fit(M, family, X, y, o, off, fi, "mixed", w=w, workspace=ws))
    assert runs["zero"]["status"].tolist() == [0, STATUS_EMPTY, 0, 0, 0]
    for kind in ("ff", "stale"):
        for f in FIELDS:
            assert bits_equal(runs[kind][f], runs["zero"][f]), (kind, f)


# ---- 7. scope ---------------------------------------------------------------------------

def test_weighted_wide_is_unsupported(M):
    """Weighted logistic at P = 193: DLSA_E_UNSUPPORTED before any launch (the
    outputs keep their fill), a DlsaHipError from Python."""
    import torch

    from dlsa_amd._hip import DlsaHipError

    n, p = 2000, 193
    X, y = O.simulate_counter(n, p, seed=1)
    X = np.ascontiguousarray(X)
    off = np.array([0, n], dtype=np.int64)
    w = np.ones(n)
    with pytest.raises(DlsaHipError, match="not supported"):
        M.logistic_model_batched_weighted(X, y, off, sample_weight=w)
    rc, out = _abi_fit(M, "dlsa_logistic_fit_batched_weighted", X, y, off, False,
                       [torch.from_numpy(w).cuda()])
    assert rc == -3  # DLSA_E_UNSUPPORTED
    for f in FIELDS:
        assert (out[f] == 7).all(), f


def test_weighted_logistic_takes_no_int8_pass(M):
    X, y, _, off = _data("logistic", 100, True)
    plain = _fit(M, "logistic", X, y, None, off, True, "mixed")
    assert plain.stats["passes_oz"] > 0  # the shape is one the int8 pass applies to
    fit = _fit(M, "logistic", X, y, None, off, True, "mixed", w=np.ones(len(y)))
    assert fit.stats["passes_oz"] == 0 and fit.stats["passes_fp64"] > 0
    assert fit.stats["passes_fp32"] > 0


# ---- 8. sharded -------------------------------------------------------------------------

@pytest.mark.parametrize("family", ["logistic", "poisson"])
def test_sharded(M, family):
    """dlsa_fit_sharded(sample_weight=) on one rank is `finish` of the reduced
    weighted fit, with N the row count."""
    from dlsa_amd.distributed import dlsa_fit_sharded, finish, loglik_sharded
    from dlsa_amd.dlsa import reduce_partitions_device, split_reduced

    p, fi = 13, True
    X, y, o, off = _data(family, p, fi)
    w = G.weights(len(y), "real")
    out = dlsa_fit_sharded(X, y, off, fit_intercept=fi, family=family, sample_weight=w,
                           rows_per_chunk=RPC, tol=TOL)
    fit = _fit(M, family, X, y, o, off, fi, "mixed", w=w)
    for f in FIELDS:
        assert bits_equal(getattr(out["fit"], f).cpu().numpy(), getattr(fit, f).cpu().numpy()), f
    S, v, st, K = split_reduced(reduce_partitions_device(fit).cpu().numpy(), fit.P)
    want = finish(S, v, st, K, int(off[-1]), fi, "lasso")
    for f in ("wlse", "oneshot", "beta_byAIC", "beta_byBIC"):
        assert _rel(out[f], want[f]) < 1e-12, f
    assert out["dbic_support"].tolist() == want["dbic_support"].tolist()
    if family == "logistic":
        betas = np.stack([out["wlse"], out["beta_byBIC"]])
        tot = loglik_sharded(X, y, off, betas, fit_intercept=fi, sample_weight=w)
        Z = G.design(X, fi)
        ref = np.array([G.loglik("logistic", Z, y, b, w) for b in betas])
        assert (np.abs(tot / ref - 1) < 1e-12).all()
