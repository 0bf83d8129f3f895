"""Poisson regression with a per-row offset on the GPU: the HIP fit
(dlsa_poisson_fit_batched_offset through models.poisson_model_batched_offset)
and evaluation pass against the numpy fp64 yardstick of
tests/_glm_ref.py.

Tolerances are those of tests/test_gpu_poisson.py: theta, Sig_inv and
Sig_inv theta within 1e-8 of the reference relative to the largest entry, the
log-likelihood within 1e-10 relative, statuses and supports exact.
"""

import numpy as np
import pytest

import _glm_ref as G
import oracle as O

pytestmark = pytest.mark.gpu

REL = 1e-8
REL_LL = 1e-10
SIZES = (3001, 1500, 4096, 2003)
NONFINITE, EMPTY, MAXITER = 4, 3, 1
FIELDS = ("theta", "sig_inv", "sig_inv_theta", "loglik", "iters", "status")


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


def _sizes(p):
    return SIZES if p <= 128 else tuple(4 * s + 1 for s in SIZES)


def _check(fit, ref, parts=None, tag="", ref_index=None):
    parts = range(fit.K) if parts is None else parts
    th, S = fit.theta.cpu().numpy(), fit.sig_inv.cpu().numpy()
    St, ll = fit.sig_inv_theta.cpu().numpy(), fit.loglik.cpu().numpy()
    for k in parts:
        j = k if ref_index is None else ref_index[k]
        e = (_rel(th[k], ref["theta"][j]), _rel(S[k], ref["sig_inv"][j]),
             _rel(St[k], ref["sig_inv_theta"][j]),
             abs(ll[k] - ref["loglik"][j]) / abs(ref["loglik"][j]))
        print(f"{tag} k={k} theta {e[0]:.2e} sig_inv {e[1]:.2e} sig_inv_theta {e[2]:.2e} "
              f"loglik {e[3]:.2e} iters {int(fit.iters[k])}")
        assert e[0] < REL and e[1] < REL and e[2] < REL
        assert e[3] < REL_LL


# ---- 1. shapes against the reference ------------------------------------------

CASES = [(1, True, "mixed"), (16, False, "mixed"), (33, False, "mixed"), (100, True, "mixed"),
         (127, True, "mixed"), (129, False, "mixed"), (192, False, "mixed"),
         (33, False, "mixed_f32"), (16, False, "fp64"), (100, True, "fp64"),
         (129, False, "fp64")]


@pytest.mark.parametrize("p,fi,hessian", CASES)
def test_shapes(M, p, fi, hessian):
    """W = 4 and W = 8 of the cooperative pass, its three precisions, both
    exact-pass kernels, the strip and no-strip per-wave geometries; chunks of
    1000 rows, so every chunk ends inside a block."""
    X, y, o, off, ref = G.case_offset(p, fi, _sizes(p))
    fit = M.poisson_model_batched_offset(X, y, off, eta_offset=o, fit_intercept=fi,
                                         hessian=hessian, rows_per_chunk=1000)
    print("stats", {k: fit.stats[k] for k in ("iterations", "passes_fp32", "passes_fp64",
                                              "passes_oz", "passes_f32x")})
    assert fit.status.cpu().numpy().tolist() == [0, 0, 0, 0]
    _check(fit, ref, tag=f"p={p} fi={fi} {hessian}")
    assert fit.stats["passes_oz"] == 0
    if hessian == "fp64":
        assert fit.stats["passes_fp32"] == 0
    else:
        assert fit.stats["passes_fp32"] > 0 and fit.stats["passes_fp64"] > 0


def test_standardised_intercept(M):
    p = 37
    off = np.concatenate([[0], np.cumsum(SIZES)]).astype(np.int64)
    n = int(off[-1])
    X, _ = G.simulate(n, p, seed=5)
    X = X * np.linspace(0.5, 3.0, p) + np.linspace(-1.0, 2.0, p)  # columns worth standardising
    center, scale = X.mean(0), X.std(0, ddof=1)
    b = np.zeros(p)
    b[:14] = 0.5
    o = np.random.default_rng(1000 + p).uniform(np.log(0.2), np.log(5.0), n)
    y = np.random.default_rng(5).poisson(
        np.exp(1.0 + ((X - center) / scale) @ (b * 0.3) + o)).astype(float)
    ref = G.fit_partitions("poisson", X, y, off, o=o, fit_intercept=True, center=center,
                           scale=scale)
    fit = M.poisson_model_batched_offset(X, y, off, eta_offset=o, fit_intercept=True,
                                         center=center, scale=scale, rows_per_chunk=1000)
    assert fit.status.cpu().numpy().tolist() == [0, 0, 0, 0]
    _check(fit, ref, tag="std p=37")


# ---- 2., 3. one iteration from the documented start point ----------------------

def _one_partition(p, fi):
    n = 3001 if p <= 128 else 12005
    X, y, o = G.simulate_offset(n, p, fit_intercept=fi)
    Z = G.design(X, fi)
    th0 = G.start("poisson", y, Z.shape[1], fi, o=o)
    step = G.newton_step("poisson", Z, y, th0, o=o)
    return X, y, o, Z, th0, step, np.array([0, n], dtype=np.int64)


def _bf16(a32):
    import torch

    t = torch.from_numpy(np.ascontiguousarray(a32, dtype=np.float32))
    return t.to(torch.bfloat16).to(torch.float64).numpy()


@pytest.mark.parametrize("p,fi", [(1, True), (16, False), (100, True), (129, False)])
def test_approximate_hessian_sees_offset(M, p, fi):
    """The converged MLE does not depend on the approximate Hessian, so a bf16
    pass that left the offset out of its weights would still pass test_shapes.
    One iteration from the start point shows it: theta_1 - theta_0 is the step
    of the bf16 image z = bf16(fl32(x) sqrt(fl32(w))), w = exp(x . theta_0 + o),
    which lies d_bf16 from the fp64 step s; a Hessian with w = exp(x . theta_0)
    lies d_wrong >= 100 d_bf16 away.  The margin of 10 is for the fp32
    accumulation and the chunked summation order (<= 1e-6 of a step).
    Measured on an MI355X, as fractions of max|s| (d_gpu, d_bf16, d_wrong):
    p = 1: 1.296e-4, 1.293e-4, 0.50; p = 16: 4.054e-4, 4.055e-4, 0.49;
    p = 100: 9.718e-4, 9.723e-4, 0.66; p = 129: 4.915e-4, 4.915e-4, 0.64."""
    X, y, o, Z, th0, s, off = _one_partition(p, fi)
    w = np.exp(Z @ th0 + o)
    g = Z.T @ (y - w)
    z = _bf16(Z.astype(np.float32) * np.sqrt(w.astype(np.float32))[:, None])
    smax = np.abs(s).max()
    d_bf16 = np.abs(np.linalg.solve(z.T @ z, g) - s).max() / smax
    w_wrong = np.exp(Z @ th0)
    d_wrong = np.abs(np.linalg.solve(Z.T @ (Z * w_wrong[:, None]), g) - s).max() / smax
    fit = M.poisson_model_batched_offset(X, y, off, eta_offset=o, fit_intercept=fi, max_iter=1,
                                         hessian="mixed")
    th1 = fit.theta[0].cpu().numpy()
    d_gpu = np.abs(th1 - th0 - s).max() / smax
    print(f"p={p} fi={fi} d_gpu {d_gpu:.3e} d_bf16 {d_bf16:.3e} d_wrong {d_wrong:.3e} "
          f"status {fit.status.cpu().numpy().tolist()} stats passes_fp32 "
          f"{fit.stats['passes_fp32']} polish {fit.stats['polish_partitions']}")
    assert d_wrong >= 100 * d_bf16  # the input condition
    assert fit.stats["passes_fp32"] == 1
    assert d_gpu <= 10 * d_bf16
    # what the polish pass publishes: Sig_inv and loglik at the returned theta
    assert fit.status.cpu().numpy().tolist() == [MAXITER]
    assert _rel(fit.sig_inv[0].cpu().numpy(), G.hessian("poisson", Z, th1, o=o)) < REL
    want = G.loglik("poisson", Z, y, th1, o=o)
    assert abs(float(fit.loglik[0]) - want) < REL_LL * abs(want)


@pytest.mark.parametrize("p,fi", [(16, False), (100, True)])
def test_start_point_and_exact_pass(M, p, fi):
    X, y, o, Z, th0, s, off = _one_partition(p, fi)
    fit = M.poisson_model_batched_offset(X, y, off, eta_offset=o, fit_intercept=fi, max_iter=1,
                                         hessian="fp64")
    th1 = fit.theta[0].cpu().numpy()
    print(f"p={p} fi={fi} theta_1 vs start + step {_rel(th1, th0 + s):.2e}")
    assert _rel(th1, th0 + s) < REL


# ---- 4. equivalences that need no reference ------------------------------------

def test_equivalences(M):
    import torch

    p, fi = 20, True
    X, y, off, _ = G.case(p, fi, SIZES)
    n = int(off[-1])
    base = M.poisson_model_batched(X, y, off, fit_intercept=fi, rows_per_chunk=1000)
    assert base.status.cpu().numpy().tolist() == [0, 0, 0, 0]

    none = M.poisson_model_batched_offset(X, y, off, fit_intercept=fi, rows_per_chunk=1000)
    for f in FIELDS:  # a null offset: the same kernels
        assert torch.equal(getattr(none, f), getattr(base, f)), f

    def close(fit, theta_want, tag):
        e = (_rel(fit.theta.cpu(), theta_want), _rel(fit.sig_inv.cpu(), base.sig_inv.cpu()),
             _rel(fit.sig_inv_theta.cpu(),
                  torch.einsum("kij,kj->ki", base.sig_inv.cpu(), torch.as_tensor(theta_want))),
             _rel(fit.loglik.cpu(), base.loglik.cpu()))
        print(tag, "theta %.2e sig_inv %.2e sig_inv_theta %.2e loglik %.2e" % e)
        assert fit.status.cpu().numpy().tolist() == [0, 0, 0, 0]
        assert e[0] < REL and e[1] < REL and e[2] < REL and e[3] < REL_LL

    zero = M.poisson_model_batched_offset(X, y, off, eta_offset=np.zeros(n), fit_intercept=fi,
                                          rows_per_chunk=1000)
    close(zero, base.theta.cpu().numpy(), "zero offset")
    print("zero offset bitwise equal:",
          {f: bool(torch.equal(getattr(zero, f), getattr(base, f))) for f in FIELDS})

    # a constant c_k per partition moves the intercept by -c_k and nothing else
    c = np.array([0.7, -1.3, 2.0, -0.25])
    shifted = base.theta.cpu().numpy().copy()
    shifted[:, 0] -= c
    const = M.poisson_model_batched_offset(X, y, off, eta_offset=np.repeat(c, np.diff(off)),
                                           fit_intercept=fi, rows_per_chunk=1000)
    close(const, shifted, "constant offset")

    # exposure = E is eta_offset = log E, the log taken on the device
    Xo, yo, oo, offo, _ = G.case_offset(p, fi, SIZES)
    E = torch.from_numpy(np.exp(oo)).to(base.theta.device)
    a = M.poisson_model_batched_offset(Xo, yo, offo, exposure=E, fit_intercept=fi,
                                       rows_per_chunk=1000)
    b = M.poisson_model_batched_offset(Xo, yo, offo, eta_offset=torch.log(E), fit_intercept=fi,
                                       rows_per_chunk=1000)
    for f in FIELDS:
        assert torch.equal(getattr(a, f), getattr(b, f)), f
    assert a.status.cpu().numpy().tolist() == [0, 0, 0, 0]


# ---- 5. a bad offset stays in its partition -------------------------------------

@pytest.mark.parametrize("hessian", ["mixed", "fp64"])
@pytest.mark.parametrize("bad", [np.nan, np.inf])
def test_bad_offset(M, bad, hessian):
    """The first row of partition 1 carries the bad offset: the last block of
    partition 0 (1500 rows: 28 of a 32-row block, 12 of a 16-row one) reads it
    as a padded row."""
    from dlsa_amd.dlsa import dlsa_mapred

    sizes, p = (1500, 2000, 2003), 8
    X, y, o, off, ref = G.case_offset(p, True, sizes)
    ob = o.copy()
    ob[off[1]] = bad
    fit = M.poisson_model_batched_offset(X, y, off, eta_offset=ob, fit_intercept=True,
                                         hessian=hessian)
    assert fit.status.cpu().numpy().tolist() == [0, NONFINITE, 0]
    _check(fit, ref, parts=[0, 2], tag=f"bad offset {bad} {hessian}")
    assert not fit.theta[1].any() and not fit.sig_inv[1].any()
    assert not fit.sig_inv_theta[1].any() and float(fit.loglik[1]) == 0.0
    assert int(fit.iters[1]) == 0
    with pytest.warns(Warning):
        comb = dlsa_mapred(fit)
    wlse, _, S = O.dlsa_mapred(ref["theta"][[0, 2]], ref["sig_inv"][[0, 2]])
    assert _rel(comb["beta_byOLS"], wlse) < REL
    assert _rel(comb.iloc[:, 2:], S) < REL


# ---- 6. warm-start level ---------------------------------------------------------

def test_warm_start_level(M):
    X, y, o, off, ref = G.case_offset(12, True, (6000, 5000))
    off3 = np.concatenate([off, off[-1:]])
    n = int(off3[-1])
    fit = M.poisson_model_batched_offset(X, y, off3, eta_offset=o, fit_intercept=True)
    print("stats", fit.stats)
    assert fit.status.cpu().numpy().tolist() == [0, 0, EMPTY]
    assert fit.stats["passes_fp32"] > 0
    assert fit.stats["rows_fp32"] < fit.stats["passes_fp32"] * n  # a row-prefix level ran
    _check(fit, ref, parts=[0, 1], tag="warm")
    assert not fit.theta[2].any() and not fit.sig_inv[2].any()


# ---- 7. evaluation -----------------------------------------------------------------

@pytest.mark.parametrize("p", [16, 200])
def test_evaluation(M, p):
    """Candidates: the fitted theta of partition 0 (the GPU fit's at p = 16;
    at p = 200, beyond the fit's limit, the reference's), 0.9 theta and zeros."""
    import torch

    sizes = (1500, 777, 2003)
    X, y, o, off, ref = G.case_offset(p, True, sizes)
    if p + 1 <= 192:
        fit = M.poisson_model_batched_offset(X, y, off, eta_offset=o, fit_intercept=True)
        th = fit.theta[0].cpu().numpy()
    else:
        fit, th = None, ref["theta"][0]
    betas = np.stack([th, 0.9 * th, np.zeros(p + 1)])
    Z = G.design(X, True)
    want = np.array([[G.loglik("poisson", Z[a:b], y[a:b], bt, o=o[a:b]) for bt in betas]
                     for a, b in zip(off[:-1], off[1:])])
    got, tot = M.poisson_loglik_batched_offset(X, y, off, betas, eta_offset=o,
                                               fit_intercept=True, return_sum=True)
    got, tot = got.cpu().numpy(), tot.cpu().numpy()
    assert got.shape == (3, 3) and tot.shape == (3,)
    print("eval rel", np.abs(got / want - 1).max(), np.abs(tot / want.sum(0) - 1).max())
    assert (np.abs(got / want - 1) < REL_LL).all()
    assert (np.abs(tot / want.sum(0) - 1) < REL_LL).all()
    fitted = float(fit.loglik[0]) if fit is not None else ref["loglik"][0]
    assert abs(got[0, 0] - fitted) < REL_LL * abs(fitted)
    # a null offset: the existing evaluation, bit for bit
    a = M.poisson_loglik_batched_offset(X, y, off, betas, fit_intercept=True)
    b = M.poisson_loglik_batched(X, y, off, betas, fit_intercept=True)
    assert torch.equal(a, b)
    # exposure is the same offset
    c = M.poisson_loglik_batched_offset(X, y, off, betas, exposure=np.exp(o), fit_intercept=True)
    assert (np.abs(c.cpu().numpy() / want - 1) < REL_LL).all()


# ---- 8. sharded ---------------------------------------------------------------------

def test_job_level(M):
    from dlsa_amd.distributed import dlsa_fit_sharded

    n, p, K, fi = 100000, 10, 4, True
    X, y, o = G.simulate_offset(n, p, fit_intercept=fi, seed=2019)
    order, off = O.systematic_partition(np.arange(n) % K)
    X, y, o = X[order], y[order], o[order]
    ref = G.fit_partitions("poisson", X, y, off, o=o, fit_intercept=fi)
    out = dlsa_fit_sharded(X, y, off, fit_intercept=fi, family="poisson", exposure=np.exp(o))
    assert out["fit"].status.cpu().numpy().tolist() == [0] * K
    wlse, _, S = O.dlsa_mapred(ref["theta"], ref["sig_inv"])
    assert _rel(out["wlse"], wlse) < REL
    _, bic = O.dlsa(S, wlse, n, fit_intercept=fi, type="lasso")
    got = set(np.nonzero(out["beta_byBIC"])[0].tolist())
    assert got == set(np.nonzero(bic)[0].tolist())
    assert got == set(range(5))
