"""The block loop of the cooperative pass at its ends, and the shapes at
which its LDS layout changes.

tests/test_gpu_coop_refill.py covers the ring's refill at five shapes on one
partition layout.  This file adds what a change to the block loop's schedule
has to survive (DESIGN.md 4.1 records the pipelined bf16 schedule that was
built against these cases, measured and not kept): chunks of one to six
32-row blocks, and more geometries of the workgroup.  A block's tile phase
lost or run twice at the loop's ends, an operand image read before it is
complete, a ring sized for another layout show as a wrong or irreproducible
Hessian: more iterations, another trajectory, a difference between two runs.
So, by the conventions of test_gpu_coop_refill (whose helpers this file
uses): every fit runs twice and must agree bit for bit, and the partitions
with a yardstick are compared with tests/_glm_ref.py at 1e-8;
rows_per_chunk = 1024.

Partitions.  Row counts 32 k - 1, 32 k, 32 k + 1 for k = 1 .. 5: chunks of 1
to 6 blocks, each with a full and a ragged last block.  Each stands between
two larger partitions of 1500 (1024 + 476: chunks of 32 and 15 blocks) and
1411 rows (1024 + 387: 32 and 13 blocks).  Which partitions have a yardstick
follows from the shape alone, by the rule of test_gpu_coop_refill: n_k >= 10 P
(logistic), n_k >= 6 P (Poisson) -- at p = 5 every Poisson partition, so
there the short chunks are checked against numpy one by one.

Shapes (p; P = p + intercept).  100: two slots, the flagship's geometry.
101: block starts at 8 mod 16.  111 + intercept: P = 112, no padding feature.
104: 27 DMA pieces per block, NT = 7.  120: NT = 8, one workgroup per CU.
140: eight waves.  16: six slots.  5.  Poisson p = 100 with offset and
weights: both row extras, the largest NT = 7 slot at that p.
"""

import functools

import numpy as np
import pytest

import _glm_ref as G
import _newton_ref as N
import test_gpu_coop_refill as R
import test_gpu_ozaki as Z

pytestmark = pytest.mark.gpu

RPC = R.RPC
SMALL = tuple(32 * k + d for k in range(1, 6) for d in (-1, 0, 1))
BIG = (1500, 1411)
SIZES = tuple(s for i, sm in enumerate(SMALL) for s in (BIG[i % 2], sm)) + (BIG[1],)
OFF = np.concatenate([[0], np.cumsum(SIZES)]).astype(np.int64)
# (p, fit_intercept)
SHAPES = [(100, False), (101, False), (111, True), (104, False), (120, False), (140, False),
          (16, False), (5, False)]
IDS = [f"p{p}{'-icpt' if fi else ''}" for p, fi in SHAPES]
ELEM = 1e-10

torch_cuda = R.torch_cuda
M = R.M


def posed(fam, P):
    need = (10 if fam == "logistic" else 6) * P
    return [k for k, s in enumerate(SIZES) if s >= need]


@functools.lru_cache(maxsize=None)
def data(fam, p, fi, std=False):
    """(X, y, center, scale) of one shape, from the generators of
    test_gpu_coop_refill.data."""
    import oracle as O

    n = int(OFF[-1])
    seed = 5000 + 7 * p + int(fi)
    if fam == "poisson":
        b = np.zeros(p)
        b[:max(1, int(0.4 * p))] = N.poisson_beta(p)
        X, y = G.simulate(n, p, seed, fit_intercept=fi, theta_true=b)
    else:
        X, y = O.simulate_counter(n, p, seed)
        X = np.ascontiguousarray(X)
    center = scale = None
    if std:
        X = X * np.linspace(0.5, 3.0, p) + np.linspace(-1.0, 2.0, p)
        center, scale = X.mean(0), X.std(0, ddof=1)
    return X, y, center, scale


@functools.lru_cache(maxsize=None)
def extras(p):
    """(offset, weights, y drawn with the offset) of the Poisson shape."""
    X, _, _, _ = data("poisson", p, False)
    n = X.shape[0]
    o = np.random.default_rng(1000 + p).uniform(np.log(0.2), np.log(5.0), n)
    b = np.zeros(p)
    b[:max(1, int(0.4 * p))] = N.poisson_beta(p)
    yo = np.random.default_rng(19).poisson(np.exp(X @ b + o)).astype(np.float64)
    return o, G.weights(n, "real"), yo


@functools.lru_cache(maxsize=None)
def yardstick(fam, p, fi, std=False, both_extras=False):
    """{k: G.fit of partition k} for the posed partitions, each converged."""
    X, y, center, scale = data(fam, p, fi, std)
    o = w = None
    if both_extras:
        o, w, y = extras(p)
    out = {}
    for k in posed(fam, p + int(fi)):
        a, b = OFF[k], OFF[k + 1]
        r = G.fit(fam, X[a:b], y[a:b], None if w is None else w[a:b],
                  None if o is None else o[a:b], fit_intercept=fi, center=center, scale=scale)
        assert r["iters"] < 50 and np.isfinite(r["theta"]).all(), (fam, p, k, r["iters"])
        out[k] = r
    return out


def _check(tag, got, ref):
    """The posed partitions against the yardstick at 1e-8, status ok."""
    assert ref, tag
    worst = 0.0
    for k, r in ref.items():
        e = (R._rel(got["theta"][k], r["theta"]), R._rel(got["sig_inv"][k], r["sig_inv"]),
             R._rel(got["sig_inv_theta"][k], r["sig_inv_theta"]),
             abs(got["loglik"][k] - r["loglik"]) / abs(r["loglik"]))
        worst = max(worst, *e)
        assert got["status"][k] == 0, (tag, k, SIZES[k], got["status"])
        assert max(e) < R.REL, (tag, k, SIZES[k], e)
    print(f"{tag}: {len(ref)} partitions against the yardstick, worst {worst:.2e}")


@pytest.mark.parametrize("p,fi", SHAPES, ids=IDS)
def test_logistic_mixed(torch_cuda, M, p, fi):
    """The bf16 passes with their digit-scale records (CM = 1, 2) where the
    int8 exact pass applies, and the exact pass behind them."""
    X, y, _, _ = data("logistic", p, fi)
    Xd, yd = R._dev(torch_cuda, X, y)
    fit, got = R._twice(lambda: M.logistic_model_batched(Xd, yd, OFF, fit_intercept=fi,
                                                         hessian="mixed", rows_per_chunk=RPC))
    print(f"logistic p={p}", {k: fit.stats[k] for k in ("passes_fp32", "passes_fp64", "passes_oz")})
    assert fit.stats["passes_fp32"] >= 2
    _check(f"logistic p={p}", got, yardstick("logistic", p, fi))


def test_poisson_short_chunks(torch_cuda, M):
    """p = 5: every partition has a yardstick, the chunks of one to six
    blocks included."""
    X, y, _, _ = data("poisson", 5, False)
    Xd, yd = R._dev(torch_cuda, X, y)
    fit, got = R._twice(lambda: M.poisson_model_batched(Xd, yd, OFF, hessian="mixed",
                                                        rows_per_chunk=RPC))
    assert fit.stats["passes_fp32"] >= 2
    ref = yardstick("poisson", 5, False)
    assert len(ref) == len(SIZES)
    _check("poisson p=5", got, ref)


def test_poisson_both_row_extras(torch_cuda, M):
    """Offset and weights at p = 100: two more DMA loads per wave and block."""
    X, _, _, _ = data("poisson", 100, False)
    o, w, yo = extras(100)
    Xd, yd, od, wd = R._dev(torch_cuda, X, yo, o, w)
    fit, got = R._twice(lambda: M.poisson_model_batched_weighted(
        Xd, yd, OFF, sample_weight=wd, eta_offset=od, hessian="mixed", rows_per_chunk=RPC))
    assert fit.stats["passes_fp32"] >= 2
    _check("poisson p=100 offset + weights", got, yardstick("poisson", 100, False, False, True))


def test_standardised(torch_cuda, M):
    X, y, center, scale = data("logistic", 100, False, True)
    Xd, yd = R._dev(torch_cuda, X, y)
    _, got = R._twice(lambda: M.logistic_model_batched(Xd, yd, OFF, center=center, scale=scale,
                                                       hessian="mixed", rows_per_chunk=RPC))
    _check("logistic p=100 std", got, yardstick("logistic", 100, False, True))


def test_mixed_against_fp64_mode(torch_cuda, M):
    """Default mode at p = 100: a max |z| record (CM = 2) and the int8 exact
    pass run; Sig_inv of the partitions with a yardstick within 1e-10 per
    entry (test_gpu_ozaki._elem) of the hessian="fp64" fit's."""
    X, y, _, _ = data("logistic", 100, False)
    Xd, yd = R._dev(torch_cuda, X, y)
    mixed = M.logistic_model_batched(Xd, yd, OFF, rows_per_chunk=RPC)
    f64 = M.logistic_model_batched(Xd, yd, OFF, hessian="fp64", rows_per_chunk=RPC)
    print({k: mixed.stats[k] for k in ("passes_fp32", "passes_fp64", "passes_oz")})
    assert mixed.stats["passes_oz"] >= 1
    ks = posed("logistic", 100)
    a, b = mixed.sig_inv.cpu().numpy()[ks], f64.sig_inv.cpu().numpy()[ks]
    assert (mixed.status.cpu().numpy()[ks] == 0).all() and (f64.status.cpu().numpy()[ks] == 0).all()
    e = Z._elem(a, b)
    print(f"Sig_inv per entry, mixed against fp64 mode: {e:.2e}")
    assert e < ELEM


@pytest.mark.parametrize("mode", ["mixed_f32", "fp64"])
def test_slot_tile_phases(torch_cuda, M, mode):
    """The fp32 / fp64 tile phases read the slot and w, r of the block."""
    X, y, _, _ = data("logistic", 100, False)
    Xd, yd = R._dev(torch_cuda, X, y)
    _, got = R._twice(lambda: M.logistic_model_batched(Xd, yd, OFF, hessian=mode,
                                                       rows_per_chunk=RPC))
    _check(f"logistic p=100 {mode}", got, yardstick("logistic", 100, False))
