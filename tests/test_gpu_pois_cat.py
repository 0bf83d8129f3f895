"""Poisson regression on the categorical-code layout, on the GPU:
dlsa_poisson_fit_categorical and dlsa_poisson_loglik_categorical through
dlsa_amd.models, the C-ABI and the sharded drivers, with a per-row offset and
prior weights in every combination.

Yardsticks: the numpy fp64 Newton of tests/_glm_ref.py on the dummy-expanded
design (oracle.expand_codes), the entry itself on row-replicated and on
collapsed data, and the library's dense weighted Poisson fit of the expanded
design.  Tolerances are the project's contracts as tests/test_gpu_cat_weighted.py
states them: theta and Sig_inv theta within 1e-8 of the largest entry, Sig_inv
per entry |d_ij| / sqrt(H_ii H_jj) < 1e-10, the log-likelihood within 1e-9
relative; statuses equal.  The fits run with tol = 1e-12 (Sig_inv is published
at the iterate before the last Newton step).

Shapes: the generator and the nine shapes of tests/test_gpu_cat_weighted.py
(three partitions of 3000-9000 rows and an empty one); drawn from the same
RandomState after beta: o ~ U(log 0.2, log 5), y ~ Poisson(exp(X beta + 0.3 + o)).

The fixed-point grids of this family are sized per pass from a bound on eta
(DESIGN 4.5h): test_grid_tightness is the one an analytic-only bound fails, and
SHAPES[4] in test_vs_numpy the marginal case; every Sig_inv comparison prints
its per-entry error per partition.
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
MASKS = ("none", "ofs", "wgt", "both")

# (q, levels, fit_intercept, standardise, rows_per_chunk): tests/test_gpu_cat_weighted.py
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


def _codes(rs, n, levels):
    return np.stack([np.minimum((L * rs.rand(n) ** 2).astype(np.int64), L - 1)
                     for L in levels], 1).astype(np.uint8) if levels else np.zeros((n, 0), np.uint8)


def _cat_case(q, levels, n_parts, seed, center=False):
    """tests/test_gpu_cat_weighted.py::_cat_case with Poisson counts and an
    offset: (Xn, codes, y, o, offsets)."""
    rs = np.random.RandomState(seed)
    sizes = [int(s) for s in rs.randint(3000, 9000, size=n_parts)]
    n = sum(sizes)
    Xn = rs.randn(n, q) * 2.0 + 1.0 if center else rs.rand(n, q) - 0.5
    codes = _codes(rs, n, levels)
    D = sum(L - 1 for L in levels)
    beta = np.concatenate([rs.uniform(-1, 1, q) * (0.5 if center else 1.0), 0.4 * rs.randn(D)])
    Xs = (Xn - 1.0) / 2.0 if center else Xn
    X = O.expand_codes(Xs, codes, levels)
    o = rs.uniform(np.log(0.2), np.log(5.0), n)
    y = rs.poisson(np.exp(X @ beta + 0.3 + o)).astype(np.float64)
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    return Xn, codes, y, o, off


def _with_empty(off):
    """An empty partition at EMPTY_AT."""
    return np.insert(off, EMPTY_AT, off[EMPTY_AT])


@functools.lru_cache(maxsize=None)
def _data(shape):
    """(Xn, codes, y, o, offsets, center, scale) of one shape, once per process."""
    q, levels, fi, std, rpc = shape
    Xn, codes, y, o, off = _cat_case(q, list(levels), 3, seed=q, center=std)
    for a in (Xn, codes, y, o):
        a.setflags(write=False)
    c = np.full(q, 1.0) if std else None
    s = np.full(q, 2.0) if std else None
    return Xn, codes, y, o, _with_empty(off), c, s


def _extras(shape, mask):
    """(o, w) of a mask: the shape's offset and the "real" weights, or None."""
    _, _, y, o, _, _, _ = _data(shape)
    return (o if mask in ("ofs", "both") else None,
            G.weights(len(y), "real") if mask in ("wgt", "both") else None)


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
def _numpy_ref(shape, mask):
    Xn, codes, y, _, off, _, _ = _data(shape)
    o, w = _extras(shape, mask)
    ref = G.fit_partitions("poisson", O.expand_codes(Xn, codes, list(shape[1])), y, off, w=w, o=o,
                           **_ref_kw(shape))
    for v in ref.values():
        v.setflags(write=False)
    return ref


def _fit(M, shape, Xn, codes, y, off, o=None, w=None, **kw):
    q, levels, fi, std, rpc = shape
    c = np.full(q, 1.0) if std else None
    s = np.full(q, 2.0) if std else None
    kw = dict(dict(fit_intercept=fi, center=c, scale=s, rows_per_chunk=rpc, tol=TOL), **kw)
    return M.poisson_model_batched_categorical(Xn, codes, y, off, list(levels), sample_weight=w,
                                               eta_offset=o, **kw)


def _compare(got, want, tag, iters_pm1=False, loglik=True):
    assert got["status"].tolist() == want["status"].tolist(), (tag, got["status"], want["status"])
    for k, st in enumerate(want["status"]):
        if st != 0:
            continue
        e = (_rel(got["theta"][k], want["theta"][k]),
             _per_entry(got["sig_inv"][k], want["sig_inv"][k]),
             _rel(got["sig_inv_theta"][k], want["sig_inv_theta"][k]),
             abs(got["loglik"][k] - want["loglik"][k]) / abs(want["loglik"][k]) if loglik else 0.0)
        print(f"{tag} k={k} theta {e[0]:.2e} sig_inv/entry {e[1]:.2e} sig_inv_theta {e[2]:.2e} "
              f"loglik {e[3]:.2e} iters {int(got['iters'][k])} vs {int(want['iters'][k])}")
        assert e[0] < REL and e[1] < REL_S and e[2] < REL and e[3] < REL_LL, (tag, k, e)
        if iters_pm1:
            assert abs(int(got["iters"][k]) - int(want["iters"][k])) <= 1, \
                (tag, k, int(got["iters"][k]), int(want["iters"][k]))


OK_STATUS = [0, STATUS_EMPTY, 0, 0]


# ---- 1. the numpy yardstick ----------------------------------------------------------------

CASES_1 = [(s, "both") for s in SHAPES] + [(SHAPES[i], m) for i in (1, 2)
                                           for m in ("none", "ofs", "wgt")]


@pytest.mark.parametrize("shape,mask", CASES_1,
                         ids=[f"{SHAPE_IDS[SHAPES.index(s)]}-{m}" for s, m in CASES_1])
def test_vs_numpy(M, shape, mask):
    Xn, codes, y, _, off, _, _ = _data(shape)
    o, w = _extras(shape, mask)
    ref = dict(_numpy_ref(shape, mask))
    assert ref["halvings"].max() <= 1 and ref["iters"].max() <= 8, (ref["iters"], ref["halvings"])
    got = _host(_fit(M, shape, Xn, codes, y, off, o=o, w=w))
    assert got["status"].tolist() == OK_STATUS
    assert got["theta"].shape[1] == int(shape[2]) + shape[0] + sum(L - 1 for L in shape[1])
    ref["status"] = got["status"]
    _compare(got, ref, f"numpy {mask} {shape[:2]}")


# ---- 2. integer omega against the entry on the replicated rows ---------------------------------

@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_replication(M, shape):
    Xn, codes, y, o, off, _, _ = _data(shape)
    w = G.weights(len(y), "int")
    got = _host(_fit(M, shape, Xn, codes, y, off, o=o, w=w))
    Xr, cr, yr, orr = G.replicate(w, Xn, codes, y, o)
    want = _host(_fit(M, shape, Xr, cr, yr, G.replicate_offsets(w, off), o=orr))
    assert want["status"].tolist() == OK_STATUS
    _compare(got, want, f"rep {shape[:2]}", iters_pm1=True)


# ---- 3. against the dense weighted path ----------------------------------------------------------

@pytest.mark.parametrize("shape", [SHAPES[2], SHAPES[3]], ids=[SHAPE_IDS[2], SHAPE_IDS[3]])
def test_vs_dense_weighted(M, shape):
    import torch

    Xn, codes, y, o, off, _, _ = _data(shape)
    w = G.weights(len(y), "real")
    got = _host(_fit(M, shape, Xn, codes, y, off, o=o, w=w))
    X = M.expand_categorical(torch.from_numpy(Xn).cuda(), torch.from_numpy(codes).cuda(),
                             list(shape[1]))
    want = _host(M.poisson_model_batched_weighted(X, y, off, sample_weight=w, eta_offset=o,
                                                  fit_intercept=shape[2], hessian="fp64",
                                                  tol=TOL))
    assert want["status"].tolist() == OK_STATUS
    _compare(got, want, f"dense {shape[:2]}", iters_pm1=True)


# ---- 4. the claim-table collapse ---------------------------------------------------------------

def test_claim_table_collapse(M):
    """q = 0, levels [6, 4, 3], intercept: raw rows with exposures e_i against
    each partition collapsed to its 72 cells with y = sum y and exposure = sum
    e.  theta, Sig_inv and Sig_inv theta agree; the log-likelihood differs by
    its constant and is not compared."""
    levels = [6, 4, 3]
    shape = (0, tuple(levels), True, False, 0)
    Xn, codes, y, o, off = _cat_case(0, levels, 3, seed=3)
    off = _with_empty(off)
    expo = np.exp(o)
    raw = _host(_fit(M, shape, Xn, codes, y, off, exposure=expo))
    assert raw["status"].tolist() == OK_STATUS
    cc, ys, es, sizes = [], [], [], []
    for a, b in zip(off[:-1], off[1:]):
        key = (codes[a:b, 0].astype(np.int64) * 4 + codes[a:b, 1]) * 3 + codes[a:b, 2]
        cells, inv = np.unique(key, return_inverse=True)
        ys.append(np.bincount(inv, weights=y[a:b], minlength=len(cells)))
        es.append(np.bincount(inv, weights=expo[a:b], minlength=len(cells)))
        cc.append(np.stack([cells // 12, cells // 3 % 4, cells % 3], 1).astype(np.uint8))
        sizes.append(len(cells))
    assert sizes == [72, 0, 72, 72], sizes  # every cell occurs in every partition
    offc = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    cells = np.concatenate(cc)
    got = _host(_fit(M, shape, np.zeros((len(cells), 0)), cells, np.concatenate(ys), offc,
                     exposure=np.concatenate(es)))
    _compare(got, raw, "collapse", iters_pm1=True, loglik=False)


# ---- 5. repeats, unit extras, None and NULL ------------------------------------------------------

def _abi_fit(shape, Xn, codes, y, o, w, off, fill=7, ws=None):
    """dlsa_poisson_fit_categorical through ctypes (o / w None: a NULL
    pointer).  Outputs pre-filled with the byte `fill`; ws: a caller workspace
    (uint8 tensor)."""
    import torch

    from dlsa_amd import _hip

    q, levels, fi, std, rpc = shape
    dev = torch.device("cuda")
    t = [None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)
         for a in (Xn, codes, y, o, w)]
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
    ptr = lambda x: None if x is None or x.numel() == 0 else ctypes.c_void_p(x.data_ptr())  # noqa: E731
    cen = torch.full((q,), 1.0, dtype=torch.float64, device=dev) if std else None
    sca = torch.full((q,), 2.0, dtype=torch.float64, device=dev) if std else None
    rc = _hip.load().dlsa_poisson_fit_categorical(
        *[ptr(x) for x in t], offs.ctypes.data_as(ctypes.c_void_p), K, q, len(levels),
        lv.ctypes.data_as(ctypes.c_void_p), int(fi), ptr(cen), ptr(sca), 100, TOL,
        *[ptr(x) for x in outs], ctypes.byref(opt),
        ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
    torch.cuda.synchronize()
    return rc, dict(zip(FIELDS, [x.cpu().numpy() for x in outs]))


@pytest.mark.parametrize("shape", [SHAPES[1], SHAPES[2], SHAPES[3]],
                         ids=[SHAPE_IDS[1], SHAPE_IDS[2], SHAPE_IDS[3]])
def test_repeats_and_unit_extras(M, shape):
    import torch

    Xn, codes, y, o, off, _, _ = _data(shape)
    w = G.weights(len(y), "real")
    a = _fit(M, shape, Xn, codes, y, off, o=o, w=w)
    b = _fit(M, shape, Xn, codes, y, off, o=o, w=w)
    for f in FIELDS:
        assert torch.equal(getattr(a, f), getattr(b, f)), f
    plain = _fit(M, shape, Xn, codes, y, off)
    hp = _host(plain)
    assert hp["status"].tolist() == OK_STATUS
    unit = _host(_fit(M, shape, Xn, codes, y, off, o=np.zeros(len(y)), w=np.ones(len(y))))
    _compare(unit, hp, f"unit {shape[:2]}")
    print(f"unit extras {shape[:2]} bitwise equal:",
          {f: bits_equal(unit[f], hp[f]) for f in FIELDS})
    rc, null = _abi_fit(shape, Xn, codes, y, None, None, off)
    assert rc == 0
    for f in FIELDS:
        assert bits_equal(null[f], hp[f]), f


# ---- 6. grid tightness ---------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _collinear_case():
    """q = 2 with columns u and u + 0.02 v, u, v ~ U(-1/2, 1/2), beta = (30,
    -30): |theta_j| m~_j is ~15 per column while eta moves by 0.3, so the
    analytic bound on eta is ~31 above its maximum."""
    levels = (4, 3)
    rs = np.random.RandomState(6)
    sizes = [int(s) for s in rs.randint(3000, 9000, size=3)]
    n = sum(sizes)
    u, v = rs.rand(n) - 0.5, rs.rand(n) - 0.5
    Xn = np.ascontiguousarray(np.stack([u, u + 0.02 * v], 1))
    codes = _codes(rs, n, levels)
    beta = np.concatenate([[30.0, -30.0], 0.4 * rs.randn(sum(L - 1 for L in levels))])
    o = rs.uniform(np.log(0.2), np.log(5.0), n)
    y = rs.poisson(np.exp(O.expand_codes(Xn, codes, levels) @ beta + 0.3 + o)).astype(np.float64)
    off = _with_empty(np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64))
    return Xn, codes, y, o, off


def test_grid_tightness(M):
    """Sig_inv per entry < 1e-10 against the numpy Hessian at the returned
    theta on a collinear design: a grid sized from the analytic bound alone is
    e^31 times too coarse here."""
    shape = (2, (4, 3), True, False, 0)
    Xn, codes, y, o, off = _collinear_case()
    w = G.weights(len(y), "real")
    got = _host(_fit(M, shape, Xn, codes, y, off, o=o, w=w))
    assert got["status"].tolist() == OK_STATUS
    X = O.expand_codes(Xn, codes, list(shape[1]))
    for k in (0, 2, 3):
        a, b = off[k], off[k + 1]
        Z = G.design(X[a:b], True)
        H = G.hessian("poisson", Z, got["theta"][k], w[a:b], o[a:b])
        e = _per_entry(got["sig_inv"][k], H)
        print(f"collinear k={k} sig_inv/entry {e:.2e} cond {np.linalg.cond(H):.1e} "
              f"iters {int(got['iters'][k])}")
        assert e < 1e-10, (k, e)


# ---- 7. a heavy row ------------------------------------------------------------------------------

def test_heavy_row_grid(M):
    """One row of one partition at omega = 1e4 and another at y = 1e5: every
    partition within 1e-10 per entry of the numpy Hessian at the returned
    theta (tests/test_gpu_cat_weighted.py::test_heavy_weight_grid).

    The heavy partition may end "maxiter" instead of "ok": its residual grid
    is sized from omega_max y_max = 1e9, so its gradient bins resolve ~1e-5 per
    term and the Newton step has a noise floor near 1e-8, above tol = 1e-12 (1
    + max|theta|); the polish pass then publishes Sig_inv at the returned
    theta, which is what is checked here.  The other partitions
    converge.  Measured: "maxiter" after 100 iterations, theta within 5.2e-9
    of numpy's, Sig_inv 6.0e-12 per entry (9.5e-15 and 1.4e-14 in the others);
    1.2e-8 with a grid sized from omega_max times the largest mu instead of
    the largest omega mu."""
    shape = SHAPES[2]
    Xn, codes, y, o, off, _, _ = _data(shape)
    w = G.weights(len(y), "real").copy()
    y = y.copy()
    k_heavy = 2  # partitions 0, (empty), 1, 2
    mid = (off[k_heavy] + off[k_heavy + 1]) // 2
    w[mid] = 1e4
    y[mid + 1] = 1e5
    got = _host(_fit(M, shape, Xn, codes, y, off, o=o, w=w))
    print("heavy row statuses", got["status"].tolist(), "iters", got["iters"].tolist())
    assert [got["status"][k] for k in (0, 1, 3)] == [0, STATUS_EMPTY, 0]
    assert got["status"][k_heavy] in (0, 1)
    X = O.expand_codes(Xn, codes, list(shape[1]))
    ref = G.fit("poisson", X[off[k_heavy]:off[k_heavy + 1]], y[off[k_heavy]:off[k_heavy + 1]],
                w[off[k_heavy]:off[k_heavy + 1]], o[off[k_heavy]:off[k_heavy + 1]],
                fit_intercept=True)
    print(f"heavy row k={k_heavy} theta vs numpy {_rel(got['theta'][k_heavy], ref['theta']):.2e}")
    for k in (0, 2, 3):
        a, b = off[k], off[k + 1]
        H = G.hessian("poisson", G.design(X[a:b], True), got["theta"][k], w[a:b], o[a:b])
        e = _per_entry(got["sig_inv"][k], H)
        print(f"heavy row k={k} sig_inv/entry {e:.2e} iters {int(got['iters'][k])}")
        assert e < 1e-10, (k, e)


# ---- 8. statuses ---------------------------------------------------------------------------------

def test_statuses(M):
    """A negative y, a NaN offset on a partition's first row, sum omega y = 0,
    one level whose rows all have omega = 0, an empty partition, and a good one
    that none of them touches."""
    from dlsa_amd import _hip

    shape = (3, (4, 3), True, False, 0)
    Xn, codes, y, o, off = _cat_case(3, [4, 3], 5, seed=17)
    off = np.insert(off, 4, off[4])  # partitions 0..3, empty 4, good 5
    n = len(y)
    w = G.weights(n, "real").copy()
    w[:off[4]] = np.maximum(w[:off[4]], 0.5)
    good_y, good_o, good_w = y.copy(), o.copy(), w.copy()
    y, o = y.copy(), o.copy()
    y[off[0] + 11] = -1.0
    o[off[1]] = np.nan  # the first row of partition 1: behind partition 0's last block
    y[off[2]:off[3]] = 0.0
    lvl = (codes[:, 1] == 2) & (np.arange(n) >= off[3]) & (np.arange(n) < off[4])
    assert lvl.sum() > 0
    w[lvl] = 0.0
    rc, got = _abi_fit(shape, Xn, codes, y, o, w, off)
    assert rc == 0, _hip.last_error()
    assert got["status"].tolist() == [STATUS_NONFINITE, STATUS_NONFINITE, STATUS_SINGULAR,
                                      STATUS_MISSING_LEVEL, STATUS_EMPTY, 0]
    for f in ("theta", "sig_inv", "sig_inv_theta", "loglik", "iters"):
        assert not got[f][:5].any(), f
    rc, clean = _abi_fit(shape, Xn, codes, good_y, good_o, good_w, off)
    assert rc == 0 and clean["status"].tolist() == [0, 0, 0, 0, STATUS_EMPTY, 0]
    for f in FIELDS:
        assert bits_equal(got[f][5], clean[f][5]), f
    # a code >= levels[f] fails the call whatever its row's weight
    bad = codes.copy()
    wz = good_w.copy()
    i = int(off[5]) + 5
    bad[i, 0], wz[i] = 4, 0.0
    rc, _ = _abi_fit(shape, Xn, bad, good_y, good_o, wz, off)
    assert rc == -1 and "level codes" in _hip.last_error()
    with pytest.raises(_hip.DlsaHipError, match="level codes"):
        _fit(M, shape, Xn, bad, good_y, off, o=good_o, w=wz)


# ---- 9. poisoned outputs and workspace -----------------------------------------------------------

@pytest.mark.parametrize("shape", [SHAPES[1], SHAPES[6]], ids=[SHAPE_IDS[1], SHAPE_IDS[6]])
def test_poisoned_outputs_and_workspace(M, shape):
    """Outputs pre-filled with 0xFF and with zeros, a 0xFF-filled caller
    workspace and none: bit-equal.  The empty partition's outputs are written
    too."""
    import torch

    Xn, codes, y, o, off, _, _ = _data(shape)
    w = G.weights(len(y), "real")
    runs = {}
    for fill in (0xFF, 0):
        for with_ws in (True, False):
            ws = torch.full((32 << 20,), 0xFF, dtype=torch.uint8, device="cuda") if with_ws \
                else None
            rc, runs[fill, with_ws] = _abi_fit(shape, Xn, codes, y, o, w, off, fill=fill, ws=ws)
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


# ---- 10. evaluation ------------------------------------------------------------------------------

def _np_loglik(shape, Xn, codes, y, off, o, w, betas):
    Z = G.design(O.expand_codes(Xn, codes, list(shape[1])), **_ref_kw(shape))
    return np.array([[G.loglik("poisson", Z[a:b], y[a:b], bt, w[a:b], o[a:b]) if b > a else 0.0
                      for bt in betas] for a, b in zip(off[:-1], off[1:])])


@pytest.mark.parametrize("B", [1, 5])
@pytest.mark.parametrize("shape,rpc", [(SHAPES[1], 700), (SHAPES[2], 1000), (SHAPES[3], 800),
                                       (SHAPES[6], 900), (SHAPES[7], 900)],
                         ids=[SHAPE_IDS[i] for i in (1, 2, 3, 6, 7)])
def test_evaluation(M, shape, rpc, B):
    """Against sum omega l in numpy (1e-12 of the largest) and against the
    dense weighted Poisson evaluation on the expanded design; partitions over
    several chunks with a ragged last block; two runs bit-equal."""
    import torch

    q, levels, fi, std, _ = shape
    Xn, codes, y, o, off, c, s = _data(shape)
    w = G.weights(len(y), "real")
    th = _numpy_ref(shape, "both")["theta"][0]
    betas = np.stack([th * f for f in (1.0, 0.9, 0.0, -0.5, 1.3)][:B])
    want = _np_loglik(shape, Xn, codes, y, off, o, w, betas)
    kw = dict(fit_intercept=fi, center=c, scale=s, rows_per_chunk=rpc, return_sum=True,
              sample_weight=w, eta_offset=o)
    got, tot = M.poisson_loglik_batched_categorical(Xn, codes, y, off, list(levels), betas, **kw)
    got2, tot2 = M.poisson_loglik_batched_categorical(Xn, codes, y, off, list(levels), betas, **kw)
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
    dense = M.poisson_loglik_batched_weighted(X, y, off, betas, sample_weight=w, eta_offset=o,
                                              fit_intercept=fi, center=rk.get("center"),
                                              scale=rk.get("scale")).cpu().numpy()
    assert np.abs(got - dense).max() < 1e-12 * np.abs(dense).max()
    # the other masks: a null offset / weight is o = 0 / omega = 1
    for mask in ("none", "ofs", "wgt"):
        om, wm = _extras(shape, mask)
        g = M.poisson_loglik_batched_categorical(
            Xn, codes, y, off, list(levels), betas, fit_intercept=fi, center=c, scale=s,
            rows_per_chunk=rpc, sample_weight=wm, eta_offset=om).cpu().numpy()
        wantm = _np_loglik(shape, Xn, codes, y, off, np.zeros(len(y)) if om is None else om,
                           np.ones(len(y)) if wm is None else wm, betas)
        assert np.abs(g - wantm).max() < 1e-12 * np.abs(wantm).max(), mask


@pytest.mark.parametrize("which", ["offset", "weight"])
def test_evaluation_nan_extra_stays_in_its_partition(M, which):
    """A NaN offset or omega on the first row of partition k + 1 -- which the
    last block of partition k's last chunk reads as a row past its end --
    leaves k's sums bit-equal and makes k + 1's non-finite."""
    import torch

    from dlsa_amd import _hip

    shape = SHAPES[1]
    q, levels, fi, std, _ = shape
    Xn, codes, y, o, off, c, s = _data(shape)
    w = G.weights(len(y), "real")
    betas = np.stack([_numpy_ref(shape, "both")["theta"][0] * f for f in (1.0, 0.5)])
    dev = torch.device("cuda")
    K = len(off) - 1
    t = {k: torch.from_numpy(np.ascontiguousarray(v)).to(dev)
         for k, v in dict(X=Xn, c=codes, y=y, b=betas, cen=c, sca=s).items()}
    lv = np.asarray(levels, dtype=np.int32)
    ptr = lambda x: ctypes.c_void_p(x.data_ptr())  # noqa: E731

    def run(ov, wv):
        od, wd = torch.from_numpy(ov).to(dev), torch.from_numpy(wv).to(dev)
        out = torch.full((K, 2), 7.0, dtype=torch.float64, device=dev)
        rc = _hip.load().dlsa_poisson_loglik_categorical(
            ptr(t["X"]), ptr(t["c"]), ptr(t["y"]), ptr(od), ptr(wd),
            off.ctypes.data_as(ctypes.c_void_p), K, q, len(levels),
            lv.ctypes.data_as(ctypes.c_void_p), int(fi), ptr(t["cen"]), ptr(t["sca"]), ptr(t["b"]),
            2, 700, ptr(out), None, ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
        assert rc == 0, _hip.last_error()
        return out.cpu().numpy()

    clean = run(o, w)
    assert np.isfinite(clean).all()
    k = 2  # partitions 0, (empty), 2, 3: the NaN goes to the first row of 3
    assert (off[k + 1] - off[k]) % 700 % 256 != 0  # a ragged last block
    ob, wb = o.copy(), w.copy()
    (ob if which == "offset" else wb)[off[k + 1]] = np.nan
    got = run(ob, wb)
    assert bits_equal(got[:k + 1], clean[:k + 1])
    assert not np.isfinite(got[k + 1]).any()


# ---- 11. sharded ---------------------------------------------------------------------------------

def test_sharded(M):
    """dlsa_fit_sharded(family="poisson", codes=, levels=, exposure=,
    sample_weight=) and loglik_sharded(family="poisson") on one rank: WLSE and
    the DBIC support equal those computed from the numpy fits."""
    from dlsa_amd.distributed import dlsa_fit_sharded, finish, loglik_sharded

    shape = SHAPES[1]
    q, levels, fi, std, rpc = shape
    Xn, codes, y, o, off, c, s = _data(shape)
    w = G.weights(len(y), "real")
    expo = np.exp(o)
    out = dlsa_fit_sharded(Xn, y, off, fit_intercept=fi, codes=codes, levels=list(levels),
                           family="poisson", exposure=expo, sample_weight=w, center=c, scale=s,
                           rows_per_chunk=rpc, tol=TOL)
    ref = _numpy_ref(shape, "both")
    parts = [k for k in range(len(off) - 1) if off[k + 1] > off[k]]
    want = finish(ref["sig_inv"][parts].sum(0), ref["sig_inv_theta"][parts].sum(0),
                  ref["theta"][parts].sum(0), len(off) - 1, int(off[-1]), fi, "lasso")
    assert _rel(out["wlse"], want["wlse"]) < REL
    assert out["dbic_support"].tolist() == want["dbic_support"].tolist()
    betas = np.stack([out["wlse"], out["beta_byBIC"]])
    tot = loglik_sharded(Xn, y, off, betas, fit_intercept=fi, center=c, scale=s, codes=codes,
                         levels=list(levels), family="poisson", exposure=expo, sample_weight=w)
    ll = _np_loglik(shape, Xn, codes, y, off, np.log(expo), w, betas).sum(0)
    assert (np.abs(tot / ll - 1) < 1e-12).all()
    # the dense evaluation's sharded form, on the expanded design
    import torch
    X = M.expand_categorical(torch.from_numpy(Xn).cuda(), torch.from_numpy(codes).cuda(),
                             list(levels))
    rk = _ref_kw(shape)
    totd = loglik_sharded(X, y, off, betas, fit_intercept=fi, center=rk.get("center"),
                          scale=rk.get("scale"), family="poisson", exposure=expo, sample_weight=w)
    assert (np.abs(totd / ll - 1) < 1e-12).all()
