"""Poisson family on the GPU: the HIP fit (dlsa_poisson_fit_batched_ex through
models.poisson_model_batched) against the numpy fp64 Newton yardstick of
tests/_glm_ref.py.

Tolerances are the project's (tests/test_gpu_parity.py): theta, Sig_inv,
Sig_invMcoef and the WLSE within 1e-8 of the reference relative to the largest
entry, the log-likelihood within 1e-10 relative, statuses and supports exact.
"""

import ctypes

import numpy as np
import pytest

import _glm_ref as G
import oracle as O

pytestmark = pytest.mark.gpu

REL = 1e-8
REL_LL = 1e-10
SIZES = (3001, 1500, 4096, 2003)
NONFINITE, SINGULAR, EMPTY = 4, 2, 3


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


def _check(fit, ref, parts=None, tag=""):
    parts = range(fit.K) if parts is None else parts
    th, S = fit.theta.cpu().numpy(), fit.sig_inv.cpu().numpy()
    St, ll = fit.sig_inv_theta.cpu().numpy(), fit.loglik.cpu().numpy()
    for k in parts:
        e = (_rel(th[k], ref["theta"][k]), _rel(S[k], ref["sig_inv"][k]),
             _rel(St[k], ref["sig_inv_theta"][k]),
             abs(ll[k] - ref["loglik"][k]) / abs(ref["loglik"][k]))
        print(f"{tag} k={k} theta {e[0]:.2e} sig_inv {e[1]:.2e} sig_inv_theta {e[2]:.2e} "
              f"loglik {e[3]:.2e} iters {int(fit.iters[k])} ref halvings {int(ref['halvings'][k])}")
        assert e[0] < REL and e[1] < REL and e[2] < REL
        assert e[3] < REL_LL


SHAPES = [(1, False), (1, True), (16, False), (33, False), (64, True), (100, True), (127, True),
          (129, False), (192, False)]
CASES = [(p, fi, "mixed") for p, fi in SHAPES] + [(16, False, "fp64"), (100, True, "fp64"),
                                                  (129, False, "fp64")]


@pytest.mark.parametrize("p,fi,hessian", CASES)
def test_shapes(M, p, fi, hessian):
    """NT = 1..12, both exact-pass kernels (per-wave up to P = 128, cooperative
    fp64 above), block tails under 8 rows, chunks of 1000 rows."""
    X, y, off, ref = G.case(p, fi, _sizes(p))
    fit = M.poisson_model_batched(X, y, off, fit_intercept=fi, hessian=hessian,
                                  rows_per_chunk=1000)
    print("stats", {k: fit.stats[k] for k in ("iterations", "passes_fp32", "passes_fp64",
                                              "passes_oz", "passes_f32x")})
    assert fit.status.cpu().numpy().tolist() == [0, 0, 0, 0]
    _check(fit, ref, tag=f"p={p} fi={fi} {hessian}")
    if hessian == "mixed" and p == 100:
        assert fit.stats["passes_oz"] == 0
        assert fit.stats["passes_fp32"] > 0 and fit.stats["passes_fp64"] > 0
    if hessian == "fp64":
        assert fit.stats["passes_fp32"] == 0


def test_halving_needed_by_reference():
    """The shapes meant to exercise the halving path do so in the reference."""
    for p in (129, 192):
        _, _, _, ref = G.case(p, False, _sizes(p))
        assert ref["halvings"].sum() >= 1


def test_standardised_intercept(M):
    p = 37
    off = np.concatenate([[0], np.cumsum(SIZES)]).astype(np.int64)
    X, _ = G.simulate(int(off[-1]), p, seed=5)
    X = X * np.linspace(0.5, 3.0, p) + np.linspace(-1.0, 2.0, p)  # columns worth standardising
    center, scale = X.mean(0), X.std(0, ddof=1)
    b = np.zeros(p)
    b[:14] = 0.5
    y = np.random.default_rng(5).poisson(np.exp(1.0 + ((X - center) / scale) @ (b * 0.3))).astype(float)
    ref = G.fit_partitions("poisson", X, y, off, fit_intercept=True, center=center, scale=scale)
    fit = M.poisson_model_batched(X, y, off, fit_intercept=True, center=center, scale=scale,
                                  rows_per_chunk=1000)
    assert fit.status.cpu().numpy().tolist() == [0, 0, 0, 0]
    _check(fit, ref, tag="std p=37")


@pytest.mark.parametrize("fi", [False, True])
def test_overshoot(M, fi):
    """mean y ~ 39 without an intercept (start theta = 0: the reference halves
    three times), ~ 57 with intercept 4.0 (where the start point matters)."""
    th = np.zeros(10)
    th[0] = 1.2
    if fi:
        X, y = G.simulate(8000, 10, seed=11, fit_intercept=True, intercept=4.0)
    else:
        X, y = G.simulate(8000, 10, seed=11, shift0=3.0, theta_true=th)
    off = np.array([0, 8000], dtype=np.int64)
    ref = G.fit_partitions("poisson", X, y, off, fit_intercept=fi)
    print("mean y", y.mean(), "ref halvings", ref["halvings"])
    if not fi:
        assert ref["halvings"][0] >= 3
    fit = M.poisson_model_batched(X, y, off, fit_intercept=fi)
    assert fit.status.cpu().numpy().tolist() == [0]
    _check(fit, ref, tag=f"overshoot fi={fi}")


@pytest.mark.parametrize("hessian", ["mixed", "fp64"])
def test_overflowing_step(M, hessian):
    """mean y ~ 1250, no intercept: the first Newton step from theta = 0 lands at
    eta ~ 1580, where exp overflows and the log-likelihood is -inf.  That is an
    overshoot to halve (the reference halves nine times), not a NONFINITE end."""
    th = np.zeros(5)
    th[0] = 2.3
    X, y = G.simulate(4000, 5, seed=13, shift0=3.0, theta_true=th)
    off = np.array([0, 4000], dtype=np.int64)
    ref = G.fit_partitions("poisson", X, y, off)
    assert ref["halvings"][0] >= 5
    fit = M.poisson_model_batched(X, y, off, hessian=hessian)
    assert fit.status.cpu().numpy().tolist() == [0]
    _check(fit, ref, tag=f"overflow {hessian}")


def test_warm_start_level(M):
    sizes = (6000, 5000, 0)
    X, y, off, ref = G.case(12, True, sizes[:2])
    off3 = np.concatenate([off, off[-1:]])
    n = int(off3[-1])
    fit = M.poisson_model_batched(X, y, off3, fit_intercept=True)
    print("stats", fit.stats)
    assert fit.status.cpu().numpy().tolist() == [0, 0, EMPTY]
    assert fit.stats["passes_fp32"] > 0
    assert fit.stats["rows_fp32"] < fit.stats["passes_fp32"] * n  # a row-prefix level ran
    _check(fit, ref, parts=[0, 1], tag="warm")
    assert not fit.theta[2].any() and not fit.sig_inv[2].any()


@pytest.mark.parametrize("order", [(0, 1, 2, 3), (2, 0, 3, 1)])
def test_bad_partitions(M, order):
    """[good, one y = -1, all y = 0, good] in two placements."""
    from dlsa_amd.dlsa import dlsa_mapred

    p, m = 8, 2000
    Xs, ys = G.simulate(4 * m, p, seed=3)
    blocks = []
    for j in range(4):
        Xb, yb = Xs[j * m:(j + 1) * m], ys[j * m:(j + 1) * m].copy()
        if j == 1:
            yb[777] = -1.0
        if j == 2:
            yb[:] = 0.0
        blocks.append((Xb, yb))
    X = np.concatenate([blocks[j][0] for j in order])
    y = np.concatenate([blocks[j][1] for j in order])
    off = np.arange(5, dtype=np.int64) * m
    want = {0: 0, 1: NONFINITE, 2: SINGULAR, 3: 0}
    good = [i for i, j in enumerate(order) if want[j] == 0]
    bad = [i for i, j in enumerate(order) if want[j] != 0]
    ref = {i: G.fit("poisson", X[off[i]:off[i + 1]], y[off[i]:off[i + 1]]) for i in good}
    fit = M.poisson_model_batched(X, y, off)
    assert fit.status.cpu().numpy().tolist() == [want[j] for j in order]
    for i in good:
        assert _rel(fit.theta[i].cpu(), ref[i]["theta"]) < REL
        assert _rel(fit.sig_inv[i].cpu(), ref[i]["sig_inv"]) < REL
        assert abs(float(fit.loglik[i]) - ref[i]["loglik"]) < REL_LL * abs(ref[i]["loglik"])
    for i in bad:
        assert not fit.theta[i].any() and not fit.sig_inv[i].any()
        assert not fit.sig_inv_theta[i].any() and float(fit.loglik[i]) == 0.0
        assert int(fit.iters[i]) == 0
    with pytest.warns(Warning):
        comb = dlsa_mapred(fit)
    wlse, _, S = O.dlsa_mapred(np.stack([ref[i]["theta"] for i in good]),
                               np.stack([ref[i]["sig_inv"] for i in good]))
    assert _rel(comb["beta_byOLS"], wlse) < REL
    assert _rel(comb.iloc[:, 2:], S) < REL


def test_limit(M):
    from dlsa_amd import DlsaHipError

    X = np.zeros((400, 193))
    y = np.ones(400)
    with pytest.raises(DlsaHipError, match="192"):
        M.poisson_model_batched(X, y, np.array([0, 400]))
    with pytest.raises(DlsaHipError, match="192"):
        M.poisson_model_batched(X[:, :192], y, np.array([0, 400]), fit_intercept=True)


def test_determinism(M):
    X, y, off, _ = G.case(100, True, SIZES)
    a = M.poisson_model_batched(X, y, off, fit_intercept=True, rows_per_chunk=1000)
    b = M.poisson_model_batched(X, y, off, fit_intercept=True, rows_per_chunk=1000)
    for f in ("theta", "sig_inv", "sig_inv_theta", "loglik", "iters", "status"):
        assert np.array_equal(getattr(a, f).cpu().numpy(), getattr(b, f).cpu().numpy()), f


@pytest.mark.parametrize("fi", [False, True])
def test_job_level(M, fi):
    from dlsa_amd.distributed import dlsa_fit_sharded

    n, p, K = 100000, 10, 4
    X, y = G.simulate(n, p, seed=2019, fit_intercept=fi)
    order, off = O.systematic_partition(np.arange(n) % K)
    X, y = X[order], y[order]
    ref = G.fit_partitions("poisson", X, y, off, fit_intercept=fi)
    out = dlsa_fit_sharded(X, y, off, fit_intercept=fi, family="poisson")
    assert out["fit"].status.cpu().numpy().tolist() == [0] * K
    wlse, _, S = O.dlsa_mapred(ref["theta"], ref["sig_inv"])
    assert _rel(out["wlse"], wlse) < REL
    _, bic = O.dlsa(S, wlse, n, fit_intercept=fi, type="lasso")
    got = set(np.nonzero(out["beta_byBIC"])[0].tolist())
    assert got == set(np.nonzero(bic)[0].tolist())
    assert got == (set(range(5)) if fi else set(range(4)))


def test_plain_c_abi(M):
    """dlsa_poisson_fit_batched_ex with a null opt."""
    import torch

    from dlsa_amd import _hip

    X, y, off, ref = G.case(10, False, SIZES)
    dev = torch.device("cuda")
    Xd, yd = torch.from_numpy(X).to(dev), torch.from_numpy(y).to(dev)
    K, P = 4, 10
    th = torch.empty((K, P), dtype=torch.float64, device=dev)
    S = torch.empty((K, P, P), dtype=torch.float64, device=dev)
    St = torch.empty((K, P), dtype=torch.float64, device=dev)
    ll = torch.empty((K,), dtype=torch.float64, device=dev)
    it = torch.empty((K,), dtype=torch.int32, device=dev)
    st = torch.empty((K,), dtype=torch.int32, device=dev)
    rc = _hip.load().dlsa_poisson_fit_batched_ex(
        Xd.data_ptr(), yd.data_ptr(), off.ctypes.data_as(ctypes.c_void_p), K, P, 0, None, None,
        100, 1e-10, th.data_ptr(), S.data_ptr(), St.data_ptr(), ll.data_ptr(), it.data_ptr(),
        st.data_ptr(), None, None)
    torch.cuda.synchronize()
    assert rc == 0, _hip.last_error()
    assert st.cpu().numpy().tolist() == [0, 0, 0, 0]
    assert _rel(th.cpu(), ref["theta"]) < REL and _rel(S.cpu(), ref["sig_inv"]) < REL
    assert _rel(St.cpu(), ref["sig_inv_theta"]) < REL
    assert _rel(ll.cpu(), ref["loglik"]) < REL_LL


@pytest.mark.parametrize("B", [3, 17])
def test_evaluation(M, B):
    p = 37
    off = np.concatenate([[0], np.cumsum(SIZES)]).astype(np.int64)
    X, y = G.simulate(int(off[-1]), p, seed=9, fit_intercept=True)
    center, scale = X.mean(0), X.std(0, ddof=1)
    rng = np.random.default_rng(B)
    betas = 0.2 * rng.standard_normal((B, p + 1))
    Z = G.design(X, True, center, scale)
    want = np.array([[G.loglik("poisson", Z[a:b], y[a:b], bt) for bt in betas]
                     for a, b in zip(off[:-1], off[1:])])
    got, tot = M.poisson_loglik_batched(X, y, off, betas, fit_intercept=True, center=center,
                                        scale=scale, return_sum=True)
    got, tot = got.cpu().numpy(), tot.cpu().numpy()
    assert got.shape == (4, B) and tot.shape == (B,)
    print("eval rel", np.abs(got / want - 1).max(), np.abs(tot / want.sum(0) - 1).max())
    assert (np.abs(got / want - 1) < REL_LL).all()
    assert (np.abs(tot / want.sum(0) - 1) < REL_LL).all()
