"""Per-row prior weights on the categorical-code layout, on the GPU:
dlsa_logistic_fit_categorical_weighted and
dlsa_logistic_loglik_categorical_weighted through dlsa_amd.models, the C-ABI
and the sharded drivers.

Yardsticks: the numpy fp64 Newton of tests/_glm_ref.py on the dummy-expanded
design, the library's own unweighted categorical fit of the row-replicated
data, and its dense weighted fit of the expanded design.  Tolerances are the
project's contracts: theta and Sig_inv theta within 1e-8 of the largest entry,
Sig_inv per entry |d_ij| / sqrt(H_ii H_jj) < 1e-10, the log-likelihood within
1e-9 relative; statuses equal.

Shapes: the generator of tests/test_gpu_parity.py::_cat_case, three partitions
of 3000-9000 rows and an empty one, at the kernel buckets of
test_categorical_vs_oracle plus the edges (an intercept without an exact
bucket: no fold factor; no numeric columns; no factors; a one-level factor).

The fits run with tol = 1e-12 for the reason in the docstring of
tests/test_gpu_weighted.py: Sig_inv is published at the iterate before the last
Newton step.
"""

import ctypes
import functools

import numpy as np
import pytest

import _glm_ref as G
import oracle as O
from _poison import STATUS_EMPTY, STATUS_NONFINITE, STATUS_SINGULAR, bits_equal

pytestmark = pytest.mark.gpu

REL = 1e-8
REL_S = 1e-10
REL_LL = 1e-9
TOL = 1e-12
STATUS_MISSING_LEVEL = 5
FIELDS = ("theta", "sig_inv", "sig_inv_theta", "loglik", "iters", "status")
EMPTY_AT = 1  # the empty partition

# (q, levels, fit_intercept, standardise, rows_per_chunk)
SHAPES = [
    (3, (4, 3), False, False, 0),                 # QN 4 bucket, no intercept
    (7, (5, 5, 9), True, True, 1500),             # QN 8, exact bucket, standardised, multi-chunk
    (9, (12, 7, 20, 30, 30), True, False, 0),     # QN 10, exact bucket (airline-like)
    (11, (3,) * 10, True, False, 0),              # QN 12, F = 10: the 16-factor kernel
    (15, (4, 6), True, True, 2000),               # QN 16, 256 threads
    (5, (4, 3), True, False, 0),                  # intercept, not an exact bucket: no fold
    (0, (6, 4), True, False, 0),                  # no numeric columns
    (5, (), True, False, 0),                      # no factors
    (3, (1, 5), False, False, 0),                 # a factor with one level (no column)
]
SHAPE_IDS = [f"q{q}-L{'x'.join(map(str, lv)) or 'none'}-{'ic' if fi else 'noic'}"
             f"{'-std' if std else ''}" for q, lv, fi, std, _ in SHAPES]


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


def _host(fit):
    return {f: getattr(fit, f).cpu().numpy() for f in FIELDS}


def _cat_case(q, levels, n_parts, seed, center=False):
    """tests/test_gpu_parity.py::_cat_case"""
    rs = np.random.RandomState(seed)
    sizes = [int(s) for s in rs.randint(3000, 9000, size=n_parts)]
    n = sum(sizes)
    Xn = rs.randn(n, q) * 2.0 + 1.0 if center else rs.rand(n, q) - 0.5
    codes = np.stack([np.minimum((L * rs.rand(n) ** 2).astype(np.int64), L - 1)
                      for L in levels], 1).astype(np.uint8) if levels else \
        np.zeros((n, 0), np.uint8)
    D = sum(L - 1 for L in levels)
    beta = np.concatenate([rs.uniform(-1, 1, q) * (0.5 if center else 1.0), 0.4 * rs.randn(D)])
    Xs = (Xn - 1.0) / 2.0 if center else Xn
    X = O.expand_codes(Xs, codes, levels)
    y = (rs.rand(n) < 1 / (1 + np.exp(-(X @ beta - 0.2)))).astype(np.float64)
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    return Xn, codes, y, off


def _with_empty(off):
    """An empty partition at EMPTY_AT."""
    return np.insert(off, EMPTY_AT, off[EMPTY_AT])


@functools.lru_cache(maxsize=None)
def _data(shape):
    """(Xn, codes, y, offsets, center, scale) of one shape, once per process."""
    q, levels, fi, std, rpc = shape
    Xn, codes, y, off = _cat_case(q, list(levels), 3, seed=q, center=std)
    c = np.full(q, 1.0) if std else None
    s = np.full(q, 2.0) if std else None
    return Xn, codes, y, _with_empty(off), c, s


def _ref_kw(shape):
    """fit_intercept / center / scale of the dummy-expanded design."""
    q, levels, fi, std, _ = shape
    D = sum(L - 1 for L in levels)
    kw = dict(fit_intercept=fi)
    if std:
        kw.update(center=np.concatenate([np.full(q, 1.0), np.zeros(D)]),
                  scale=np.concatenate([np.full(q, 2.0), np.ones(D)]))
    return kw


@functools.lru_cache(maxsize=None)
def _numpy_ref(shape, kind):
    Xn, codes, y, off, _, _ = _data(shape)
    w = G.weights(len(y), kind)
    ref = G.fit_partitions("logistic", O.expand_codes(Xn, codes, list(shape[1])), y, off, w=w,
                           **_ref_kw(shape))
    for v in ref.values():
        v.setflags(write=False)
    return ref


def _fit(M, shape, Xn, codes, y, off, w=None, **kw):
    """w None: the unweighted entry as it stands; else the weighted one."""
    q, levels, fi, std, rpc = shape
    c = np.full(q, 1.0) if std else None
    s = np.full(q, 2.0) if std else None
    kw = dict(fit_intercept=fi, center=c, scale=s, rows_per_chunk=rpc, tol=TOL, **kw)
    if w is None:
        return M.logistic_model_batched_categorical(Xn, codes, y, off, list(levels), **kw)
    return M.logistic_model_batched_categorical_weighted(Xn, codes, y, off, list(levels),
                                                         sample_weight=w, **kw)


def _compare(got, want, tag, iters_pm1=False):
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


OK_STATUS = [0, STATUS_EMPTY, 0, 0]


# ---- 1. real omega against the numpy yardstick ---------------------------------------

@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_real_weights_vs_numpy(M, shape):
    Xn, codes, y, off, _, _ = _data(shape)
    w = G.weights(len(y), "real")
    ref = dict(_numpy_ref(shape, "real"))
    assert ref["halvings"].max() == 0 and ref["iters"].max() <= 8, (ref["iters"], ref["halvings"])
    got = _host(_fit(M, shape, Xn, codes, y, off, w=w))
    assert got["status"].tolist() == OK_STATUS
    assert got["theta"].shape[1] == int(shape[2]) + shape[0] + sum(L - 1 for L in shape[1])
    ref["status"] = got["status"]
    _compare(got, ref, f"real {shape[:2]}")


# ---- 2. integer omega and "spread" against the code as it stands ------------------------

@pytest.mark.parametrize("kind", ["int", "spread"])
@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_replication(M, shape, kind):
    """The weighted fit of the n rows against the unweighted categorical entry
    on the replicated rows (omega = 0 left out).  No warm-start level on either
    side: the code layout runs one only from 2^19 rows per partition."""
    Xn, codes, y, off, _, _ = _data(shape)
    w = G.weights(len(y), kind)
    got = _host(_fit(M, shape, Xn, codes, y, off, w=w))
    Xr, cr, yr = G.replicate(w, Xn, codes, y)
    want = _host(_fit(M, shape, Xr, cr, yr, G.replicate_offsets(w, off)))
    assert want["status"].tolist() == OK_STATUS
    _compare(got, want, f"rep {kind} {shape[:2]}", iters_pm1=True)


# ---- 3. against the dense weighted path ----------------------------------------------------

@pytest.mark.parametrize("shape", [SHAPES[2], SHAPES[3]], ids=[SHAPE_IDS[2], SHAPE_IDS[3]])
def test_vs_dense_weighted(M, shape):
    """An exact-bucket shape and a 16-factor-kernel shape against
    logistic_model_batched_weighted on expand_categorical."""
    import torch

    Xn, codes, y, off, _, _ = _data(shape)
    w = G.weights(len(y), "real")
    got = _host(_fit(M, shape, Xn, codes, y, off, w=w))
    X = M.expand_categorical(torch.from_numpy(Xn).cuda(), torch.from_numpy(codes).cuda(),
                             list(shape[1]))
    want = _host(M.logistic_model_batched_weighted(X, y, off, sample_weight=w,
                                                   fit_intercept=shape[2], hessian="fp64",
                                                   tol=TOL))
    assert want["status"].tolist() == OK_STATUS
    _compare(got, want, f"dense {shape[:2]}", iters_pm1=True)


# ---- 4. the contingency-table collapse --------------------------------------------------

def test_contingency_table_collapse(M):
    """q = 0, levels [6, 4, 3], intercept: each partition's 0/1 rows collapsed
    to its 72 cells (s successes of m rows): the weighted fit of the
    72-row partitions, y = s / m and omega = m, is the unweighted fit of
    the raw rows."""
    levels = [6, 4, 3]
    shape = (0, tuple(levels), True, False, 0)
    Xn, codes, y, off = _cat_case(0, levels, 3, seed=3)
    off = _with_empty(off)
    raw = _host(_fit(M, shape, Xn, codes, y, off))
    assert raw["status"].tolist() == OK_STATUS
    cc, ys, ms, sizes = [], [], [], []
    for a, b in zip(off[:-1], off[1:]):
        key = (codes[a:b, 0].astype(np.int64) * 4 + codes[a:b, 1]) * 3 + codes[a:b, 2]
        cells, inv = np.unique(key, return_inverse=True)
        m = np.bincount(inv, minlength=len(cells)).astype(np.float64)
        s = np.bincount(inv, weights=y[a:b], minlength=len(cells))
        cc.append(np.stack([cells // 12, cells // 3 % 4, cells % 3], 1).astype(np.uint8))
        ys.append(s / m)
        ms.append(m)
        sizes.append(len(cells))
    assert sizes == [72, 0, 72, 72], sizes  # every cell occurs in every partition
    offc = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    cells = np.concatenate(cc)
    got = _host(_fit(M, shape, np.zeros((len(cells), 0)), cells, np.concatenate(ys), offc,
                     w=np.concatenate(ms)))
    print("cells per partition", sizes)
    _compare(got, raw, "collapse", iters_pm1=True)


# ---- 5. repeats, omega = 1, None and NULL --------------------------------------------------

@pytest.mark.parametrize("shape", [SHAPES[1], SHAPES[2], SHAPES[3]],
                         ids=[SHAPE_IDS[1], SHAPE_IDS[2], SHAPE_IDS[3]])
def test_repeats_and_unit_weights(M, shape):
    import torch

    Xn, codes, y, off, _, _ = _data(shape)
    w = G.weights(len(y), "real")
    a = _fit(M, shape, Xn, codes, y, off, w=w)
    b = _fit(M, shape, Xn, codes, y, off, w=w)
    for f in FIELDS:
        assert torch.equal(getattr(a, f), getattr(b, f)), f
    base = _fit(M, shape, Xn, codes, y, off)
    ones = _host(_fit(M, shape, Xn, codes, y, off, w=np.ones(len(y))))
    hb = _host(base)
    assert hb["status"].tolist() == OK_STATUS
    _compare(ones, hb, f"unit {shape[:2]}")
    print(f"unit weights {shape[:2]} bitwise equal:",
          {f: bits_equal(ones[f], hb[f]) for f in FIELDS})
    none = _fit(M, shape, Xn, codes, y, off, w=None)
    viaw = M.logistic_model_batched_categorical_weighted(
        Xn, codes, y, off, list(shape[1]), None, fit_intercept=shape[2],
        center=None if not shape[3] else np.full(shape[0], 1.0),
        scale=None if not shape[3] else np.full(shape[0], 2.0), rows_per_chunk=shape[4], tol=TOL)
    for f in FIELDS:
        assert torch.equal(getattr(viaw, f), getattr(none, f)), f


# ---- 6. the grids under a heavy weight --------------------------------------------------

def test_heavy_weight_grid(M):
    """One row of partition 1 (the second non-empty one) at omega = 1e4: the
    grids of that partition are 1e4 times coarser, and still every partition's
    Sig_inv is within 1e-10 per entry of the numpy Hessian at the returned
    theta."""
    shape = SHAPES[2]
    Xn, codes, y, off, _, _ = _data(shape)
    w = G.weights(len(y), "real").copy()
    k_heavy = 2  # partitions 0, (empty), 1, 2
    w[(off[k_heavy] + off[k_heavy + 1]) // 2] = 1e4
    got = _host(_fit(M, shape, Xn, codes, y, off, w=w))
    assert got["status"].tolist() == OK_STATUS
    X = O.expand_codes(Xn, codes, list(shape[1]))
    for k in (0, 2, 3):
        a, b = off[k], off[k + 1]
        H = G.hessian("logistic", G.design(X[a:b], True), got["theta"][k], w[a:b])
        e = _per_entry(got["sig_inv"][k], H)
        print(f"heavy weight k={k} sig_inv/entry {e:.2e}")
        assert e < 1e-10, (k, e)


# ---- 7. statuses ------------------------------------------------------------------------------

def _abi_fit(shape, Xn, codes, y, w, off, fill=7, ws=None, entry=None):
    """dlsa_logistic_fit_categorical_weighted through ctypes (w None: a NULL
    row_weight; entry: another symbol without the weight argument).  Outputs
    pre-filled with the byte `fill`; ws: a caller workspace (uint8 tensor)."""
    import torch

    from dlsa_amd import _hip

    q, levels, fi, std, rpc = shape
    dev = torch.device("cuda")
    Xd = torch.from_numpy(np.ascontiguousarray(Xn)).to(dev)
    cd = torch.from_numpy(np.ascontiguousarray(codes)).to(dev)
    yd = torch.from_numpy(y).to(dev)
    wd = None if w is None else torch.from_numpy(w).to(dev)
    K = len(off) - 1
    P = int(fi) + q + sum(L - 1 for L in levels)
    outs = [torch.full((n,), fill, dtype=torch.uint8, device=dev).view(dt).reshape(s)
            for n, dt, s in ((8 * K * P, torch.float64, (K, P)),
                             (8 * K * P * P, torch.float64, (K, P, P)),
                             (8 * K * P, torch.float64, (K, P)), (8 * K, torch.float64, (K,)),
                             (4 * K, torch.int32, (K,)), (4 * K, torch.int32, (K,)))]
    opt = _hip.default_options()
    opt.rows_per_chunk = rpc
    if ws is not None:
        opt.workspace = ws.data_ptr()
        opt.workspace_bytes = ws.numel()
    offs = np.ascontiguousarray(off, dtype=np.int64)
    lv = np.asarray(levels, dtype=np.int32)
    ptr = lambda t: None if t is None or t.numel() == 0 else ctypes.c_void_p(t.data_ptr())  # noqa: E731
    cen = torch.full((q,), 1.0, dtype=torch.float64, device=dev) if std else None
    sca = torch.full((q,), 2.0, dtype=torch.float64, device=dev) if std else None
    extra = [ptr(wd)] if entry is None else []
    rc = getattr(_hip.load(), entry or "dlsa_logistic_fit_categorical_weighted")(
        ptr(Xd), ptr(cd), ptr(yd), *extra, offs.ctypes.data_as(ctypes.c_void_p), K, q,
        len(levels), lv.ctypes.data_as(ctypes.c_void_p), int(fi), ptr(cen), ptr(sca), 100, TOL,
        *[ptr(t) for t in outs], ctypes.byref(opt),
        ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
    torch.cuda.synchronize()
    return rc, dict(zip(FIELDS, [t.cpu().numpy() for t in outs]))


def test_statuses(M):
    """A negative omega, a NaN omega, all omega = 0, one level whose rows all
    have omega = 0, an empty partition, and a good one that none of them
    touches."""
    from dlsa_amd import _hip

    shape = (3, (4, 3), True, False, 0)
    Xn, codes, y, off = _cat_case(3, [4, 3], 5, seed=17)
    off = np.insert(off, 4, off[4])  # partitions 0..3, empty 4, good 5
    n = len(y)
    w = G.weights(n, "real").copy()
    good = w.copy()
    good[:off[4]] = 1.0
    w[off[0] + 11] = -0.5
    w[off[1]] = np.nan  # the first row of partition 1: behind partition 0's last block
    w[off[2]:off[3]] = 0.0
    lvl = (codes[:, 1] == 2) & (np.arange(n) >= off[3]) & (np.arange(n) < off[4])
    assert lvl.sum() > 0 and (w[off[3]:off[4]] > 0).sum() > lvl.sum()
    w[lvl] = 0.0
    with pytest.raises(ValueError, match="sample_weight"):  # the Python layer refuses it
        _fit(M, shape, Xn, codes, y, off, w=w)
    rc, got = _abi_fit(shape, Xn, codes, y, w, off)
    assert rc == 0, _hip.last_error()
    assert got["status"].tolist() == [STATUS_NONFINITE, STATUS_NONFINITE, STATUS_SINGULAR,
                                      STATUS_MISSING_LEVEL, STATUS_EMPTY, 0]
    for f in ("theta", "sig_inv", "sig_inv_theta", "loglik", "iters"):
        assert not got[f][:5].any(), f
    rc, clean = _abi_fit(shape, Xn, codes, y, good, off)
    assert rc == 0 and clean["status"].tolist() == [0, 0, 0, 0, STATUS_EMPTY, 0]
    for f in FIELDS:
        assert bits_equal(got[f][5], clean[f][5]), f
    # a code >= levels[f] fails the call whatever its row's weight
    bad = codes.copy()
    wz = good.copy()
    i = int(off[5]) + 5
    bad[i, 0], wz[i] = 4, 0.0
    rc, _ = _abi_fit(shape, Xn, bad, y, wz, off)
    assert rc == -1 and "level codes" in _hip.last_error()
    with pytest.raises(_hip.DlsaHipError, match="level codes"):
        _fit(M, shape, Xn, bad, y, off, w=wz)


# ---- 8. poisoned outputs and workspace --------------------------------------------------------

@pytest.mark.parametrize("shape", [SHAPES[1], SHAPES[6]], ids=[SHAPE_IDS[1], SHAPE_IDS[6]])
def test_poisoned_outputs_and_workspace(M, shape):
    """Outputs pre-filled with 0xFF and with zeros, a 0xFF-filled caller
    workspace and none: bit-equal.  The empty partition's outputs are written
    too."""
    import torch

    Xn, codes, y, off, _, _ = _data(shape)
    w = G.weights(len(y), "real")
    runs = {}
    for fill in (0xFF, 0):
        for with_ws in (True, False):
            ws = torch.full((32 << 20,), 0xFF, dtype=torch.uint8, device="cuda") if with_ws \
                else None
            rc, runs[fill, with_ws] = _abi_fit(shape, Xn, codes, y, w, off, fill=fill, ws=ws)
            assert rc == 0
            if with_ws:  # large enough, so it was the one used
                assert bool((ws != 0xFF).any())
    first = runs[0xFF, True]
    assert first["status"].tolist() == OK_STATUS
    for f in ("theta", "sig_inv", "sig_inv_theta", "loglik", "iters"):
        assert not first[f][EMPTY_AT].any(), f
    for key, r in runs.items():
        for f in FIELDS:
            assert bits_equal(r[f], first[f]), (key, f)
    # and a NULL row_weight is the unweighted entry, bit for bit
    rc, null = _abi_fit(shape, Xn, codes, y, None, off)
    rc2, plain = _abi_fit(shape, Xn, codes, y, None, off, entry="dlsa_logistic_fit_categorical")
    assert rc == 0 and rc2 == 0
    for f in FIELDS:
        assert bits_equal(null[f], plain[f]), f


# ---- 9. evaluation ------------------------------------------------------------------------------

def _np_loglik(shape, Xn, codes, y, off, w, betas):
    Z = G.design(O.expand_codes(Xn, codes, list(shape[1])), **_ref_kw(shape))
    return np.array([[G.loglik("logistic", Z[a:b], y[a:b], bt, w[a:b]) if b > a else 0.0
                      for bt in betas] for a, b in zip(off[:-1], off[1:])])


@pytest.mark.parametrize("B", [1, 5])
@pytest.mark.parametrize("shape,rpc", [(SHAPES[1], 700), (SHAPES[2], 1000), (SHAPES[3], 0),
                                       (SHAPES[6], 900), (SHAPES[7], 900)],
                         ids=[SHAPE_IDS[i] for i in (1, 2, 3, 6, 7)])
def test_evaluation(M, shape, rpc, B):
    """Weighted evaluation against sum omega l in numpy (1e-12 of the largest)
    and against the dense weighted evaluation on the expanded design;
    partitions over several chunks with a ragged last block; two runs
    bit-equal."""
    import torch

    q, levels, fi, std, _ = shape
    Xn, codes, y, off, c, s = _data(shape)
    w = G.weights(len(y), "real")
    th = _numpy_ref(shape, "real")["theta"][0]
    betas = np.stack([th * f for f in (1.0, 0.9, 0.0, -0.5, 1.3)][:B])
    want = _np_loglik(shape, Xn, codes, y, off, w, betas)
    kw = dict(fit_intercept=fi, center=c, scale=s, rows_per_chunk=rpc, return_sum=True,
              sample_weight=w)
    got, tot = M.logistic_loglik_batched_categorical(Xn, codes, y, off, list(levels), betas, **kw)
    got2, tot2 = M.logistic_loglik_batched_categorical(Xn, codes, y, off, list(levels), betas,
                                                       **kw)
    assert torch.equal(got, got2) and torch.equal(tot, tot2)
    got, tot = got.cpu().numpy(), tot.cpu().numpy()
    assert got.shape == (len(off) - 1, B) and not got[EMPTY_AT].any()
    e = (np.abs(got - want).max() / np.abs(want).max(),
         np.abs(tot - want.sum(0)).max() / np.abs(want.sum(0)).max())
    print(f"eval {shape[:2]} B={B}: per partition {e[0]:.2e} summed {e[1]:.2e}")
    assert e[0] < 1e-12 and e[1] < 1e-12
    X = M.expand_categorical(torch.from_numpy(Xn).cuda(), torch.from_numpy(codes).cuda(),
                             list(levels))
    rk = _ref_kw(shape)
    dense = M.logistic_loglik_batched(X, y, off, betas, fit_intercept=fi,
                                      center=rk.get("center"), scale=rk.get("scale"),
                                      sample_weight=w).cpu().numpy()
    assert np.abs(got - dense).max() < 1e-12 * np.abs(dense).max()


def test_evaluation_nan_weight_stays_in_its_partition(M):
    """A NaN omega on the first row of partition k + 1 -- which the last block
    of partition k's last chunk reads as a row past its end -- leaves k's sums
    bit-equal and makes k + 1's non-finite."""
    import torch

    from dlsa_amd import _hip

    shape = SHAPES[1]
    q, levels, fi, std, _ = shape
    Xn, codes, y, off, c, s = _data(shape)
    w = G.weights(len(y), "real").copy()
    betas = np.stack([_numpy_ref(shape, "real")["theta"][0] * f for f in (1.0, 0.5)])
    dev = torch.device("cuda")
    K, P = len(off) - 1, betas.shape[1]
    t = {k: torch.from_numpy(np.ascontiguousarray(v)).to(dev)
         for k, v in dict(X=Xn, c=codes, y=y, b=betas, cen=c, sca=s).items()}
    lv = np.asarray(levels, dtype=np.int32)
    ptr = lambda x: ctypes.c_void_p(x.data_ptr())  # noqa: E731

    def run(wv):
        wd = torch.from_numpy(wv).to(dev)
        out = torch.full((K, 2), 7.0, dtype=torch.float64, device=dev)
        rc = _hip.load().dlsa_logistic_loglik_categorical_weighted(
            ptr(t["X"]), ptr(t["c"]), ptr(t["y"]), ptr(wd), off.ctypes.data_as(ctypes.c_void_p),
            K, q, len(levels), lv.ctypes.data_as(ctypes.c_void_p), int(fi), ptr(t["cen"]),
            ptr(t["sca"]), ptr(t["b"]), 2, 700, ptr(out), None,
            ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
        assert rc == 0, _hip.last_error()
        return out.cpu().numpy()

    clean = run(w)
    assert np.isfinite(clean).all()
    k = 2  # partitions 0, (empty), 2, 3: the NaN goes to the first row of 3
    assert (off[k + 1] - off[k]) % 700 % 256 != 0  # a ragged last block
    wb = w.copy()
    wb[off[k + 1]] = np.nan
    got = run(wb)
    assert bits_equal(got[:k + 1], clean[:k + 1])
    assert not np.isfinite(got[k + 1]).any()


# ---- 10. sharded --------------------------------------------------------------------------------

def test_sharded(M):
    """dlsa_fit_sharded(codes=, levels=, sample_weight=) and loglik_sharded on
    one rank: WLSE and the DBIC support equal those computed from the numpy
    weighted fits."""
    from dlsa_amd.distributed import dlsa_fit_sharded, finish, loglik_sharded

    shape = SHAPES[1]
    q, levels, fi, std, rpc = shape
    Xn, codes, y, off, c, s = _data(shape)
    w = G.weights(len(y), "real")
    out = dlsa_fit_sharded(Xn, y, off, fit_intercept=fi, codes=codes, levels=list(levels),
                           sample_weight=w, center=c, scale=s, rows_per_chunk=rpc, tol=TOL)
    ref = _numpy_ref(shape, "real")
    parts = [k for k in range(len(off) - 1) if off[k + 1] > off[k]]
    want = finish(ref["sig_inv"][parts].sum(0), ref["sig_inv_theta"][parts].sum(0),
                  ref["theta"][parts].sum(0), len(off) - 1, int(off[-1]), fi, "lasso")
    assert _rel(out["wlse"], want["wlse"]) < REL
    assert out["dbic_support"].tolist() == want["dbic_support"].tolist()
    betas = np.stack([out["wlse"], out["beta_byBIC"]])
    tot = loglik_sharded(Xn, y, off, betas, fit_intercept=fi, center=c, scale=s, codes=codes,
                         levels=list(levels), sample_weight=w)
    ll = _np_loglik(shape, Xn, codes, y, off, w, betas).sum(0)
    assert (np.abs(tot / ll - 1) < 1e-12).all()
