"""Routing of the cooperative and per-wave passes by column-tile count: every
NT = 1..12 of every family's units (logistic, OLS, Poisson, Poisson with a
per-row offset), approximate and exact Hessians, against the yardstick and the
tolerances of each family's own shape test (test_gpu_parity.py
test_shapes_vs_oracle and test_ols_vs_oracle, test_gpu_poisson.py and
test_gpu_poisson_offset.py test_shapes).

One P per NT in (16 (NT - 1), 16 NT], the intercept on the odd NT: a full last
tile (32, 64, 128, 160, 192), the two strip geometries of the per-wave pass
(P = 67: 3 rows of the last tile, P = 88: 8) and ragged ones.  Two ragged
partitions of the shape tests' sizes (four times as many rows above P = 128,
where n / P must stay above the MLE-existence threshold), chunks of 1000 rows,
so every chunk ends inside a block.
"""

import functools

import numpy as np
import pytest

import _glm_ref as G
import oracle as O

pytestmark = pytest.mark.gpu

REL = 1e-8
REL_LL = 1e-10
P_OF_NT = {1: 13, 2: 32, 3: 37, 4: 64, 5: 67, 6: 88, 7: 100, 8: 128, 9: 129, 10: 160, 11: 165,
           12: 192}
NTS = sorted(P_OF_NT)


def _shape(NT):
    """(p, fit_intercept, partition sizes) of tile count NT."""
    P = P_OF_NT[NT]
    assert 16 * (NT - 1) < P <= 16 * NT
    fi = NT % 2 == 1
    return P - fi, fi, ((3001, 1500) if P <= 128 else (12005, 6001))


def _rel(a, b):
    a = np.asarray(a, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)


@pytest.fixture(scope="module")
def M():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a visible MI355X"
    from dlsa_amd import models
    return models


def _offsets(sizes):
    return np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)


def _usable(ref, iters, max_iter):
    """The yardstick converged, with finite values, in every partition."""
    return (np.asarray(iters) < max_iter).all() and all(
        np.isfinite(ref[k]).all() for k in ("theta", "sig_inv", "sig_inv_theta", "loglik"))


@functools.lru_cache(maxsize=None)
def logistic_case(NT):
    p, fi, sizes = _shape(NT)
    off = _offsets(sizes)
    X, y = O.simulate_counter(int(off[-1]), p, seed=p * 7 + fi)
    th, S, St, ll, it = O.logistic_fit_partitions(X, y, off, fit_intercept=fi)
    ref = {"theta": th, "sig_inv": S, "sig_inv_theta": St, "loglik": ll}
    assert _usable(ref, it, 100)
    return X, y, off, ref


@functools.lru_cache(maxsize=None)
def ols_case(NT):
    p, fi, sizes = _shape(NT)
    off = _offsets(sizes)
    rs = np.random.RandomState(p)
    n = int(off[-1])
    X = rs.rand(n, p) - 0.5
    y = X @ rs.randn(p) + 0.3 + 0.1 * rs.randn(n)
    return X, y, off


def poisson_case(NT):
    p, fi, sizes = _shape(NT)
    X, y, off, ref = G.case(p, fi, sizes)
    assert _usable(ref, ref["iters"], 200)
    return X, y, off, ref


def poisson_offset_case(NT):
    p, fi, sizes = _shape(NT)
    X, y, o, off, ref = G.case_offset(p, fi, sizes)
    assert _usable(ref, ref["iters"], 200)
    return X, y, o, off, ref


def _check(fit, ref, tag):
    assert fit.status.cpu().numpy().tolist() == [0, 0]
    e = (_rel(fit.theta.cpu(), ref["theta"]), _rel(fit.sig_inv.cpu(), ref["sig_inv"]),
         _rel(fit.sig_inv_theta.cpu(), ref["sig_inv_theta"]),
         np.abs(fit.loglik.cpu().numpy() / ref["loglik"] - 1).max())
    print(f"{tag} theta {e[0]:.2e} sig_inv {e[1]:.2e} sig_inv_theta {e[2]:.2e} loglik {e[3]:.2e} "
          f"passes fp32 {fit.stats['passes_fp32']} fp64 {fit.stats['passes_fp64']} "
          f"oz {fit.stats['passes_oz']}")
    assert e[0] < REL and e[1] < REL and e[2] < REL
    assert e[3] < REL_LL


def _check_passes(fit, hessian):
    if hessian == "fp64":
        assert fit.stats["passes_fp32"] == 0 and fit.stats["passes_fp64"] > 0
    else:
        assert fit.stats["passes_fp32"] > 0 and fit.stats["passes_fp64"] > 0


@pytest.mark.parametrize("hessian", ["mixed", "fp64"])
@pytest.mark.parametrize("NT", NTS)
def test_logistic(M, NT, hessian):
    p, fi, _ = _shape(NT)
    X, y, off, ref = logistic_case(NT)
    fit = M.logistic_model_batched(X, y, off, fit_intercept=fi, hessian=hessian,
                                   rows_per_chunk=1000)
    _check(fit, ref, f"logistic NT={NT} p={p} fi={fi} {hessian}")
    _check_passes(fit, hessian)


@pytest.mark.parametrize("NT", NTS)
def test_ols(M, NT):
    p, fi, _ = _shape(NT)
    X, y, off = ols_case(NT)
    fit = M.ols_model_batched(X, y, off, fit_intercept=fi, rows_per_chunk=1000)
    assert fit.status.cpu().numpy().tolist() == [0, 0]
    for k in range(2):
        Xk, yk = X[off[k]:off[k + 1]], y[off[k]:off[k + 1]]
        o = O.ols_fit(Xk, yk, fit_intercept=fi)
        assert np.isfinite(o["coef"]).all() and np.isfinite(o["Sig_inv"]).all()
        if fi:
            Xk = np.column_stack([np.ones(len(Xk)), Xk])
        rss = float(((yk - Xk @ o["coef"]) ** 2).sum())
        e = (_rel(fit.theta[k].cpu(), o["coef"]), _rel(fit.sig_inv[k].cpu(), o["Sig_inv"]),
             abs(fit.loglik[k].item() - rss) / rss)
        print(f"ols NT={NT} p={p} fi={fi} k={k} theta {e[0]:.2e} sig_inv {e[1]:.2e} rss {e[2]:.2e}")
        assert e[0] < REL
        assert e[1] < 1e-12
        assert e[2] < 1e-6


@pytest.mark.parametrize("hessian", ["mixed", "fp64"])
@pytest.mark.parametrize("NT", NTS)
def test_poisson(M, NT, hessian):
    p, fi, _ = _shape(NT)
    X, y, off, ref = poisson_case(NT)
    fit = M.poisson_model_batched(X, y, off, fit_intercept=fi, hessian=hessian,
                                  rows_per_chunk=1000)
    _check(fit, ref, f"poisson NT={NT} p={p} fi={fi} {hessian}")
    _check_passes(fit, hessian)
    assert fit.stats["passes_oz"] == 0


@pytest.mark.parametrize("hessian", ["mixed", "fp64"])
@pytest.mark.parametrize("NT", NTS)
def test_poisson_offset(M, NT, hessian):
    p, fi, _ = _shape(NT)
    X, y, o, off, ref = poisson_offset_case(NT)
    fit = M.poisson_model_batched_offset(X, y, off, eta_offset=o, fit_intercept=fi,
                                         hessian=hessian, rows_per_chunk=1000)
    _check(fit, ref, f"poisson offset NT={NT} p={p} fi={fi} {hessian}")
    _check_passes(fit, hessian)
    assert fit.stats["passes_oz"] == 0
