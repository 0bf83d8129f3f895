"""The piece schedule of the cooperative pass: a block's KiB pieces, y and the
row extras are each DMA'd once, and a launch whose blocks all start 16-byte
aligned (p even, X aligned) with p % 4 == 0 fetches no piece behind the block.

Two schedules exist, chosen per launch from X's address and p: the exact one
(aligned; for p % 4 == 0 one piece fewer per block, nothing of the next block
in the slot) and the fallback (a block may start at 8 mod 16, one more piece
where the span needs it).  They move different bytes into differently sized
slots -- for some shapes into rings of different depth -- and must give the
same bits.  What can go wrong: a wave waiting on the wrong count (a slot read
before it landed), a row stream placed or issued wrongly, the bytes behind a
block no longer finite.  It shows as a wrong sum, a difference between two
runs or two schedules, or a non-finite partition.  So, with the helpers and
rules of tests/test_gpu_coop_refill.py (rows_per_chunk = 1024, every fit run
twice and bit-equal, the posed partitions against tests/_glm_ref.py at 1e-8):

Partitions of 31, 32, 33, 63, 64 and 65 rows (one and two blocks, full, one
row short, one row over), each between two of 1500 and 1411 rows (1024 + 476
and 1024 + 387: two chunks, more blocks than slots, ragged ends).  The large
ones have a yardstick at every p here (n_k >= 10 P up to P = 132; Poisson
n_k >= 6 P); the short ones end in whatever status their data earn (31 rows
against 100 parameters is no MLE) and must only be reproducible, equal under
both schedules and untouched by their neighbours.

Shapes: p = 100 (the flagship's slot), 16, 64, 112 (P = PMAX: no padding
feature), 132 with hessian="fp64" (the cooperative fp64 pass, eight waves), 98
(p % 4 == 2: both runs take today's count, the aligned one with s = 0), and 84
(the aligned launch gets a three-slot ring where the fallback has two).
"""

import functools

import numpy as np
import pytest

import _glm_ref as G
import _newton_ref as N
import test_gpu_coop_refill as R
import test_gpu_newton_steps as T
from test_gpu_coop_refill import M, torch_cuda  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu

RPC = R.RPC
FIELDS = R.FIELDS
SHORT = (31, 32, 33, 63, 64, 65)
SIZES = (1500, 31, 1411, 32, 1500, 33, 1411, 63, 1500, 64, 1411, 65, 1500)
OFF = np.concatenate([[0], np.cumsum(SIZES)]).astype(np.int64)
SHORT_K = tuple(k for k, s in enumerate(SIZES) if s in SHORT)
NONFINITE = R.NONFINITE
# (p, hessian)
SHAPES = [(100, "mixed"), (16, "mixed"), (64, "mixed"), (112, "mixed"), (132, "fp64"),
          (98, "mixed")]
CHANGED_SLOTS = (84, "mixed")  # NT = 6: 2 slots (fallback) -> 3 (exact)


def _id(s):
    return f"p{s[0]}-{s[1]}"


@functools.lru_cache(maxsize=None)
def data(fam, p):
    import oracle as O

    n = int(OFF[-1])
    seed = 5000 + 7 * p
    if fam == "poisson":
        b = np.zeros(p)
        b[:max(1, int(0.4 * p))] = N.poisson_beta(p)
        X, y = G.simulate(n, p, seed, theta_true=b)
    else:
        X, y = O.simulate_counter(n, p, seed)
    return np.ascontiguousarray(X, dtype=np.float64), np.ascontiguousarray(y, dtype=np.float64)


def posed(fam, P):
    need = (10 if fam == "logistic" else 6) * P
    return [k for k, s in enumerate(SIZES) if s >= need]


@functools.lru_cache(maxsize=None)
def yardstick(fam, p, extras=False):
    X, y = data(fam, p)
    o = w = None
    if extras:
        o, w, y = row_extras(p)
    out = {}
    for k in posed(fam, p):
        a, b = OFF[k], OFF[k + 1]
        r = G.fit(fam, X[a:b], y[a:b], None if w is None else w[a:b],
                  None if o is None else o[a:b])
        assert r["iters"] < 50 and np.isfinite(r["theta"]).all(), (fam, p, k, r["iters"])
        out[k] = r
    return out


@functools.lru_cache(maxsize=None)
def row_extras(p):
    """(offset, weights, y drawn with the offset) of the Poisson shape."""
    X, _ = data("poisson", p)
    n = X.shape[0]
    o = np.random.default_rng(1000 + p).uniform(np.log(0.2), np.log(5.0), n)
    b = np.zeros(p)
    b[:max(1, int(0.4 * p))] = N.poisson_beta(p)
    yo = np.random.default_rng(17).poisson(np.exp(X @ b + o)).astype(np.float64)
    return o, G.weights(n, "real"), yo


def _check(tag, got, ref):
    """The posed partitions against the yardstick at 1e-8, status ok."""
    assert ref, tag
    for k, r in ref.items():
        e = (R._rel(got["theta"][k], r["theta"]), R._rel(got["sig_inv"][k], r["sig_inv"]),
             R._rel(got["sig_inv_theta"][k], r["sig_inv_theta"]),
             abs(got["loglik"][k] - r["loglik"]) / abs(r["loglik"]))
        print(f"{tag} k={k} n_k={SIZES[k]} status {got['status'][k]} iters {got['iters'][k]}: "
              f"theta {e[0]:.2e} sig_inv {e[1]:.2e} sig_inv_theta {e[2]:.2e} loglik {e[3]:.2e}")
        assert got["status"][k] == 0, (tag, k, got["status"])
        assert max(e) < R.REL, (tag, k, e)


def _placed(torch, X, shift, tail=0):
    """X [n, p] as a contiguous view of a flat device buffer, `shift` doubles
    from its start (the allocation is at least 16-byte aligned: shift 0 is an
    aligned X, shift 1 one at 8 mod 16) and `tail` doubles of NaN behind it."""
    n, p = X.shape
    flat = torch.full((shift + n * p + tail,), float("nan"), dtype=torch.float64, device="cuda")
    assert flat.data_ptr() % 16 == 0
    v = flat[shift:shift + n * p].view(n, p)
    v.copy_(torch.from_numpy(X))
    assert v.is_contiguous() and v.data_ptr() % 16 == 8 * (shift % 2)
    return v


def _both_schedules(torch, M, p, mode):
    """The logistic fit of the shape from an aligned X and from one at 8 mod
    16, each run twice: bit-equal, and the posed partitions at 1e-8."""
    X, y = data("logistic", p)
    yd, = R._dev(torch, y)
    got = []
    for shift in (0, 1):
        Xd = _placed(torch, X, shift)
        fit, g = R._twice(lambda: M.logistic_model_batched(Xd, yd, OFF, hessian=mode,
                                                           rows_per_chunk=RPC))
        print(f"p={p} {mode} X at {8 * shift} mod 16: status", g["status"].tolist(),
              {k: fit.stats[k] for k in ("passes_fp32", "passes_fp64", "passes_oz")})
        got.append(g)
    for f in FIELDS:
        assert got[0][f].tobytes() == got[1][f].tobytes(), f"p={p}: {f} differs between the schedules"
    _check(f"logistic p={p} {mode}", got[0], yardstick("logistic", p))
    return got[0]


@pytest.mark.parametrize("shape", SHAPES, ids=_id)
def test_two_schedules_one_answer(torch_cuda, M, shape):
    """(a) the exact and the fallback schedule give the same bits."""
    _both_schedules(torch_cuda, M, *shape)


def test_changed_slot_count(torch_cuda, M):
    """(d) p = 84: the exact slot is a KiB smaller and a third one fits the
    workgroup's LDS share; the fallback launch of the same data has two."""
    _both_schedules(torch_cuda, M, *CHANGED_SLOTS)


def _poison(X):
    """Every row of the partition behind each short one: NaN, +inf, -inf and
    1e300 in turn."""
    Xn = X.copy()
    vals = np.array([np.nan, np.inf, -np.inf, 1e300])
    bad = [k + 1 for k in SHORT_K]
    for k in bad:
        a, b = int(OFF[k]), int(OFF[k + 1])
        Xn[a:b] = vals[np.arange((b - a) * X.shape[1]) % 4].reshape(b - a, -1)
    return Xn, bad


@pytest.mark.parametrize("shape", [s for s in SHAPES if s[0] % 4 == 0], ids=_id)
def test_nothing_behind_the_block_matters(torch_cuda, M, shape):
    """(b) the rows behind a short partition (in its last block's DMA under the
    fallback, in no DMA under the exact schedule) and the pad behind the block
    leave it alone: with those rows NaN / +-inf / 1e300 the short partitions
    are bit for bit what they were.  Their status is what the clean run gave
    them -- it is part of the compared fields -- and never "nonfinite"; it is
    "ok" only where the clean data earn it (31 rows and 100 parameters have no
    MLE with or without the neighbour)."""
    p, mode = shape
    X, y = data("logistic", p)
    yd, = R._dev(torch_cuda, y)
    clean = R._arrays(M.logistic_model_batched(_placed(torch_cuda, X, 0), yd, OFF, hessian=mode,
                                               rows_per_chunk=RPC))
    Xn, bad = _poison(X)
    Xnd = _placed(torch_cuda, Xn, 0)
    _, got = R._twice(lambda: M.logistic_model_batched(Xnd, yd, OFF, hessian=mode,
                                                       rows_per_chunk=RPC))
    print(f"p={p} status", got["status"].tolist(), "clean", clean["status"].tolist())
    for k in range(len(SIZES)):
        if k in bad:
            assert got["status"][k] == NONFINITE, (k, got["status"])
            continue
        assert got["status"][k] != NONFINITE, (k, got["status"])
        for f in FIELDS:
            assert got[f][k].tobytes() == clean[f][k].tobytes(), (p, k, f)
    assert got["status"][0] == 0


@pytest.mark.parametrize("shift", [0, 1], ids=["aligned", "8mod16"])
def test_allocation_ends_at_the_last_row(torch_cuda, M, shift):
    """(b) X ends with its buffer and the last partition has 33 rows (its
    second block holds one row): the same bits as from a buffer with NaN
    behind the last row."""
    p, sizes = 100, (1500, 33)
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    X, y = data("logistic", p)
    X, y = X[:off[-1]], y[:off[-1]]
    yd, = R._dev(torch_cuda, y)
    Xe = _placed(torch_cuda, X, shift)
    assert Xe.untyped_storage().nbytes() == (shift + X.size) * 8  # no slack behind the last row
    _, exact = R._twice(lambda: M.logistic_model_batched(Xe, yd, off, rows_per_chunk=RPC))
    Xs = _placed(torch_cuda, X, shift, tail=64 * p)
    slack = R._arrays(M.logistic_model_batched(Xs, yd, off, rows_per_chunk=RPC))
    print("status", exact["status"].tolist())
    for f in FIELDS:
        assert exact[f].tobytes() == slack[f].tobytes(), f
    assert exact["status"][0] == 0 and exact["status"][1] != NONFINITE
    r = G.fit("logistic", X[:1500], y[:1500])
    assert R._rel(exact["theta"][0], r["theta"]) < R.REL
    assert R._rel(exact["sig_inv"][0], r["sig_inv"]) < R.REL


def test_poisson_offset_and_weights(torch_cuda, M):
    """(c) both row extras at p = 100, the largest NT = 7 slot: y, the offset
    and the weight are three items of three different waves."""
    p = 100
    X, _ = data("poisson", p)
    o, w, yo = row_extras(p)
    Xd, yd, od, wd = R._dev(torch_cuda, X, yo, o, w)
    run = lambda **kw: M.poisson_model_batched_weighted(  # noqa: E731
        Xd, yd, OFF, sample_weight=wd, eta_offset=od, hessian="mixed", rows_per_chunk=RPC, **kw)
    _, got = R._twice(run)
    _check("poisson p=100 offset + weights", got, yardstick("poisson", p, True))
    # max_iter = 1 from theta = 0: the bf16 Newton step of the emulator's
    # operands (tests/_newton_ref.py: hessian, bf16_image) with the weights
    # omega exp(o), within a tenth of the one-row defect D_1 (the rule of
    # tests/test_gpu_newton_steps.py)
    th1 = run(max_iter=1).theta.cpu().numpy()
    for k in posed("poisson", p):
        a, b = OFF[k], OFF[k + 1]
        D = N.Design(X[a:b])
        mu = np.exp(o[a:b])
        wk = w[a:b] * mu
        g = D.Z.T @ (w[a:b] * (yo[a:b] - mu))
        d = np.linalg.solve(N.hessian(D, wk, "bf16"), g)
        dm = np.abs(np.linalg.solve(N.hessian(D, wk, "bf16", drop_last=True), g) - d).max()
        e = {"theta": d, "s": float(np.abs(d).max()), "D": float(dm)}
        dist = np.abs(th1[k] - d).max()
        print(f"poisson extras k={k} max_iter=1: dist/D {dist / dm:.2e} (s {e['s']:.2e})")
        assert dist <= T._tolerance(e, False), (k, dist, dm)


def test_logistic_mixed_f32(torch_cuda, M):
    """(c) the fp32 tile phase reads x from the slot to the end of the block."""
    p = 100
    X, y = data("logistic", p)
    Xd, yd = R._dev(torch_cuda, X, y)
    run = lambda **kw: M.logistic_model_batched(Xd, yd, OFF, hessian="mixed_f32",  # noqa: E731
                                                rows_per_chunk=RPC, **kw)
    _, got = R._twice(run)
    _check("logistic p=100 mixed_f32", got, yardstick("logistic", p))
    th1 = run(max_iter=1).theta.cpu().numpy()
    for k in posed("logistic", p):
        a, b = OFF[k], OFF[k + 1]
        ys, _ = N.step_yardsticks(N.Design(X[a:b]), y[a:b], "logistic", False, "mixed_f32", 1, RPC)
        T._check_iterate(f"logistic mixed_f32 k={k}", th1[k], ys[0], False)
