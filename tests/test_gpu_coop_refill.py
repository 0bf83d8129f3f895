"""The LDS ring of the cooperative pass at the ring's edges.

A ring slot is refilled by LDS-DMA at barrier B1 of the block after the one
that read it, while the other slots are in flight or being read; the bf16
tile phase runs the last wave's surplus tile entries without a branch.  What
can go wrong in code like this (and in any other refill schedule: DESIGN.md
4.1 records the one that was measured and not kept) is a slot written while it
is read, or read before it landed: it shows as a wrong sum, a difference
between two runs of the same fit, or a non-finite partition.  So every fit
here runs twice and must agree bit for bit, and the well-posed partitions are
compared with the numpy yardstick (tests/_glm_ref.py) at the suite's 1e-8.

Shapes.  p = 100 (two slots, the flagship's geometry), 101 (odd: block starts
at 8 mod 16), 111 + intercept (P = 112, no padding feature), 16 (six slots),
5.  rows_per_chunk = 1024; partitions of 1, 31, 32, 33, 64, 65 and 1027 rows
(chunks of 1, 2, 3 and 32 blocks, ragged last blocks, more blocks than slots
and fewer) between two larger ones (1500 rows: 1024 + 476, ends mid-block;
2085: 2 x 1024 + 37).  The first partition has 33 rows: it ends mid-block and
the DMA of its last block brings in its neighbour's rows.

Which partitions have a yardstick.  A logistic MLE needs rows well beyond P
(below it the classes separate), a Poisson one exists from a few rows per
parameter on: n_k >= 10 P (the rule of tests/_newton_ref.py) for the logistic
fits, n_k >= 6 P for the Poisson ones -- from the shape alone.  The yardstick
of such a partition must itself have converged (asserted).  The other
partitions (down to one row) end in whatever status their data earn; they
must only be reproducible and leave their neighbours alone.
"""

import functools

import numpy as np
import pytest

import _glm_ref as G
import _newton_ref as N
import test_gpu_newton_steps as T

pytestmark = pytest.mark.gpu

REL = 1e-8
RPC = 1024
SIZES = (33, 1500, 1, 31, 32, 1027, 64, 65, 2085)
OFF = np.concatenate([[0], np.cumsum(SIZES)]).astype(np.int64)
NONFINITE = 4
# (p, fit_intercept)
SHAPES = [(100, False), (101, False), (111, True), (16, False), (5, False)]
FIELDS = ("theta", "sig_inv", "sig_inv_theta", "loglik", "iters", "status")


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a visible MI355X"
    return torch


@pytest.fixture(scope="module")
def M(torch_cuda):
    from dlsa_amd import models
    return models


def _rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)


def posed(fam, P):
    """Indices of the partitions that have a yardstick (module docstring)."""
    need = (10 if fam == "logistic" else 6) * P
    return [k for k, s in enumerate(SIZES) if s >= need]


@functools.lru_cache(maxsize=None)
def data(fam, p, fi, std=False):
    """(X, y, center, scale) of one shape; the generators of the suite's
    other GLM cases (tests/_newton_ref.py case_data)."""
    import oracle as O

    n = int(OFF[-1])
    seed = 3000 + 7 * p + int(fi)
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
    """(offset, weights, y) of the Poisson shape with row extras: o = log
    exposure ~ U(log 0.2, log 5), omega ~ U(0.2, 5) with exact zeros, y drawn
    with the offset."""
    X, _, _, _ = data("poisson", p, False)
    n = X.shape[0]
    o = np.random.default_rng(1000 + p).uniform(np.log(0.2), np.log(5.0), n)
    b = np.zeros(p)
    b[:max(1, int(0.4 * p))] = N.poisson_beta(p)
    yo = np.random.default_rng(17).poisson(np.exp(X @ b + o)).astype(np.float64)
    return o, G.weights(n, "real"), yo


@functools.lru_cache(maxsize=None)
def yardstick(fam, p, fi, std=False, extra=None):
    """{k: G.fit of partition k} for the posed partitions, each converged."""
    X, y, center, scale = data(fam, p, fi, std)
    o = w = None
    if extra is not None:
        oo, ww, yo = extras(p)
        o, w = (oo, None) if extra == "offset" else (None, ww)
        y = yo if extra == "offset" else y
    out = {}
    for k in posed(fam, p + int(fi)):
        a, b = OFF[k], OFF[k + 1]
        r = G.fit(fam, X[a:b], y[a:b], None if w is None else w[a:b],
                  None if o is None else o[a:b], fit_intercept=fi, center=center, scale=scale)
        assert r["iters"] < 50 and np.isfinite(r["theta"]).all(), (fam, p, k, r["iters"])
        out[k] = r
    return out


def _arrays(fit):
    return {f: getattr(fit, f).cpu().numpy() for f in FIELDS}


def _twice(run):
    """The fit's outputs, run twice: bit-identical (NaN bits included)."""
    f1 = run()
    a, b = _arrays(f1), _arrays(run())
    for f in FIELDS:
        assert a[f].tobytes() == b[f].tobytes(), f"{f} differs between two runs of one fit"
    return f1, a


def _check(tag, got, ref):
    """The posed partitions against the yardstick at 1e-8, status ok."""
    assert ref, tag
    for k, r in ref.items():
        e = (_rel(got["theta"][k], r["theta"]), _rel(got["sig_inv"][k], r["sig_inv"]),
             _rel(got["sig_inv_theta"][k], r["sig_inv_theta"]),
             abs(got["loglik"][k] - r["loglik"]) / abs(r["loglik"]))
        print(f"{tag} k={k} n_k={SIZES[k]} status {got['status'][k]} iters {got['iters'][k]}: "
              f"theta {e[0]:.2e} sig_inv {e[1]:.2e} sig_inv_theta {e[2]:.2e} loglik {e[3]:.2e}")
        assert got["status"][k] == 0, (tag, k, got["status"])
        assert max(e) < REL, (tag, k, e)


def _dev(torch, *arrs):
    return [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in arrs]


@pytest.mark.parametrize("p,fi", SHAPES, ids=[f"p{p}{'-icpt' if fi else ''}" for p, fi in SHAPES])
def test_logistic_mixed(torch_cuda, M, p, fi):
    """bf16 passes with both digit-scale records (CM = 1, 2) and the int8
    exact pass behind them."""
    X, y, _, _ = data("logistic", p, fi)
    Xd, yd = _dev(torch_cuda, X, y)
    fit, got = _twice(lambda: M.logistic_model_batched(Xd, yd, OFF, fit_intercept=fi,
                                                       hessian="mixed", rows_per_chunk=RPC))
    print(f"logistic p={p}", "status", got["status"].tolist(),
          {k: fit.stats[k] for k in ("passes_fp32", "passes_fp64", "passes_oz")})
    assert fit.stats["passes_fp32"] >= 2
    if p == 100:
        assert fit.stats["passes_oz"] >= 1
    _check(f"logistic p={p}", got, yardstick("logistic", p, fi))


@pytest.mark.parametrize("p,fi", SHAPES, ids=[f"p{p}{'-icpt' if fi else ''}" for p, fi in SHAPES])
def test_poisson_mixed(torch_cuda, M, p, fi):
    X, y, _, _ = data("poisson", p, fi)
    Xd, yd = _dev(torch_cuda, X, y)
    fit, got = _twice(lambda: M.poisson_model_batched(Xd, yd, OFF, fit_intercept=fi,
                                                      hessian="mixed", rows_per_chunk=RPC))
    print(f"poisson p={p}", "status", got["status"].tolist())
    assert fit.stats["passes_fp32"] >= 2
    _check(f"poisson p={p}", got, yardstick("poisson", p, fi))


def test_standardised(torch_cuda, M):
    X, y, center, scale = data("logistic", 100, False, True)
    Xd, yd = _dev(torch_cuda, X, y)
    _, got = _twice(lambda: M.logistic_model_batched(Xd, yd, OFF, center=center, scale=scale,
                                                     hessian="mixed", rows_per_chunk=RPC))
    _check("logistic p=100 std", got, yardstick("logistic", 100, False, True))


@pytest.mark.parametrize("mode", ["mixed_f32", "fp64"])
def test_slot_read_by_the_tile_phase(torch_cuda, M, mode):
    """The fp32 / fp64 tile phases read x from the slot, to the end of the
    block."""
    X, y, _, _ = data("logistic", 100, False)
    Xd, yd = _dev(torch_cuda, X, y)
    _, got = _twice(lambda: M.logistic_model_batched(Xd, yd, OFF, hessian=mode,
                                                     rows_per_chunk=RPC))
    _check(f"logistic p=100 {mode}", got, yardstick("logistic", 100, False))


@pytest.mark.parametrize("extra", ["offset", "weights"])
def test_poisson_row_extras(torch_cuda, M, extra):
    """One more DMA load per wave and block behind y."""
    X, y, _, _ = data("poisson", 100, False)
    o, w, yo = extras(100)
    if extra == "offset":
        Xd, yd, od = _dev(torch_cuda, X, yo, o)
        run = lambda: M.poisson_model_batched_offset(Xd, yd, OFF, eta_offset=od,  # noqa: E731
                                                     hessian="mixed", rows_per_chunk=RPC)
    else:
        Xd, yd, wd = _dev(torch_cuda, X, y, w)
        run = lambda: M.poisson_model_batched_weighted(Xd, yd, OFF, sample_weight=wd,  # noqa: E731
                                                       hessian="mixed", rows_per_chunk=RPC)
    _, got = _twice(run)
    _check(f"poisson p=100 {extra}", got, yardstick("poisson", 100, False, False, extra))


@pytest.mark.parametrize("fam", ["logistic", "poisson"])
def test_nan_neighbour(torch_cuda, M, fam):
    """Every row of X NaN in the 31-row partition (the 1500-row one ends
    mid-block 28 rows into its last block, then comes the 1-row partition:
    that block's DMA brings 3 of the NaN rows into the slot) and in the 64-row
    one (behind the 3-row last chunk of the 1027-row partition, ahead of the
    65-row one): they end nonfinite, every other partition is bit for bit what
    it is without them.  (Not the 1-row partition itself: a Poisson partition
    with sum y = 0 is SINGULAR before any pass looks at X.)"""
    X, y, _, _ = data(fam, 100, False)
    model = M.logistic_model_batched if fam == "logistic" else M.poisson_model_batched
    Xd, yd = _dev(torch_cuda, X, y)
    clean = _arrays(model(Xd, yd, OFF, hessian="mixed", rows_per_chunk=RPC))
    bad = (3, 6)
    Xn = X.copy()
    for k in bad:
        Xn[OFF[k]:OFF[k + 1]] = np.nan
    Xnd, = _dev(torch_cuda, Xn)
    _, got = _twice(lambda: model(Xnd, yd, OFF, hessian="mixed", rows_per_chunk=RPC))
    print(fam, "status", got["status"].tolist(), "clean", clean["status"].tolist())
    for k in range(len(SIZES)):
        if k in bad:
            assert got["status"][k] == NONFINITE, (k, got["status"])
        else:
            for f in FIELDS:
                assert got[f][k].tobytes() == clean[f][k].tobytes(), (fam, k, f)
    _check(f"{fam} p=100 NaN neighbours", got, yardstick(fam, 100, False))


def test_iterates_p100(torch_cuda, M):
    """theta after max_iter = 1, 2, 3 at P = 100 (no intercept: the flagship's
    slot layout) against the emulator, by the rule and the code of
    tests/test_gpu_newton_steps.py."""
    T._run_case(torch_cuda, M, ("logistic", "mixed", 100, False, False), False)
