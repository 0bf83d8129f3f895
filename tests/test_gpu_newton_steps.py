"""The Newton iterates of the batched fits against the emulator of
tests/_newton_ref.py: the passes that steer the fit (cooperative bf16 pass,
its fp32-MFMA variant, wide fused bf16 pass) and the state machine around
them, checked where they act -- at theta after max_iter = m iterations, which
the polish pass does not move -- instead of at the fixed point only.

Every partition has n_k <= max(2048, 64 P) rows, so no warm-start row-prefix
level runs: a fit is max_iter full-data iterations from the start point
(asserted from the stats).

Tolerance of theta_m, from the reference alone (tests/test_cpu_newton_ref.py
checks what it rests on for every case here):
  mixed, mixed_f32   0.1 D_m, D_m = the distance by which leaving ONE row
                     (the partition's last) out of the Hessian of iteration m
                     moves theta_m; the modelled fp32 accumulation noise of a
                     correct pass is <= 0.01 D_m;
  fp64, categorical  1e-8 s_m, s_m = max |theta_m - theta_{m-1}| (the
                     project's REL; every pass is exact),
each plus 1e-13 (1 + max |theta_m|), the resolution of a converged fp64
iterate (it matters only where a partition has converged within m: s_m ~
1e-16).  Each check prints the measured distance in units of s_m and D_m.

What theta_m is compared with.  theta_1, every iterate of the exact modes and
every halved iterate: the emulator's own iterate.  An approximate step from m
= 2 on: the emulator's step FROM THE FIT'S OWN theta_{m-1} (the fit with
max_iter = m - 1; the fits are deterministic), in the phase the emulated
trajectory is in.  The accumulation noise of iteration m - 1 (~1e-7 s) moves
the weights of iteration m by about an fp32 ulp, which flips a handful of the
n P bf16 roundings of the image -- 2^-8 of an entry each, chaotic, and
measured at up to 0.03 D_m (modelled: _newton_ref.step_yardsticks,
"carried").  From the same theta_{m-1} both sides round the same numbers, the
distance is back at the accumulation noise, and by induction over m the whole
trajectory is pinned.  The distance to the emulator's own trajectory is
printed next to it.
"""

import numpy as np
import pytest

import _glm_ref as G
import _newton_ref as N

pytestmark = pytest.mark.gpu

REL = 1e-8
REL_LL = 1e-10
DEFECT_FRACTION = 0.1
FLOOR = 1e-13
OK, MAXITER = 0, 1


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
    a = np.asarray(a, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)


def _tolerance(e, exact):
    t = REL * e["s"] if exact else DEFECT_FRACTION * e["D"]
    return t + FLOOR * (1.0 + np.abs(e["theta"]).max())


def _check_iterate(tag, th_gpu, e, exact, step_from=None):
    """theta of one partition against the emulated iterate `e`, or against the
    emulator's step from `step_from` = (Design, y, family, the fit's own
    previous iterate) where that is given and the iteration took a step."""
    want = e["theta"]
    traj = np.abs(th_gpu - want).max()
    if step_from is not None and not exact and not e["rec"]["halved"]:
        D, y, fam, prev = step_from
        want = N.newton_step(D, y, fam, prev, e["rec"]["hmode"])
    dist = np.abs(th_gpu - want).max()
    print(f"{tag} m={e['rec']['it']} {e['rec']['hmode']}: dist/s {dist / e['s']:.2e} "
          f"dist/D {dist / e['D']:.2e} (s {e['s']:.2e}, D/s {e['D'] / e['s']:.2e}; "
          f"to the emulated trajectory: /s {traj / e['s']:.2e} /D {traj / e['D']:.2e})")
    assert dist <= _tolerance(e, exact), (tag, dist, e["s"], e["D"])


def _expected_passes(ys, m, nk):
    """(iters, status) per partition and (passes_fp32, rows_fp32, exact passes
    before the polish) of a fit stopped after m iterations, from the
    emulator's phases."""
    iters, status = [], []
    p32 = rows32 = p64 = 0
    for it in range(1, m + 1):
        approx = [k for k, (st, _) in enumerate(ys) if len(st) >= it and st[it - 1]["rec"]["phase"]
                  != N.PHASE_F64]
        exact = [k for k, (st, _) in enumerate(ys) if len(st) >= it and st[it - 1]["rec"]["phase"]
                 == N.PHASE_F64]
        p32 += bool(approx)
        rows32 += sum(int(nk[k]) for k in approx)
        p64 += bool(exact)
    for st, tr in ys:
        done = tr["status"] == "ok" and len(st) <= m
        iters.append(len(st) if done else m)
        status.append(OK if done else MAXITER)
    return iters, status, p32, rows32, p64


def _eval_at(fam, X, y, theta, fi, center, scale):
    """fp64 numpy Sig_inv, Sig_inv theta and log-likelihood at a given theta."""
    Z = G.design(X, fi, center, scale)
    eta = Z @ theta
    _, w = N.weights(fam, eta)
    S = Z.T @ (Z * w[:, None])
    ll = G.loglik("poisson", Z, y, theta) if fam == "poisson" else N.loglik(fam, eta, y)
    return S, S @ theta, ll


def _check_outputs_at_theta(tag, fit, fam, X, y, off, fi, center, scale, parts=None):
    th = fit.theta.cpu().numpy()
    for k in (range(len(off) - 1) if parts is None else parts):
        a, b = off[k], off[k + 1]
        S, St, ll = _eval_at(fam, X[a:b], y[a:b], th[k], fi, center, scale)
        e = (_rel(fit.sig_inv[k].cpu(), S), _rel(fit.sig_inv_theta[k].cpu(), St),
             abs(float(fit.loglik[k]) - ll) / abs(ll))
        print(f"{tag} k={k} at theta: sig_inv {e[0]:.2e} sig_inv_theta {e[1]:.2e} loglik {e[2]:.2e}")
        assert e[0] < REL and e[1] < REL and e[2] < REL_LL, (tag, k, e)


def _dense_fit(M, fam):
    return M.poisson_model_batched if fam == "poisson" else M.logistic_model_batched


def _run_case(torch, M, case, wide):
    fam, mode, p, fi, std = case
    X, y, off, center, scale = N.case_data(fam, p, fi, std, wide)
    ys = N.case_yardsticks(fam, mode, p, fi, std, wide)
    nk, K, n = np.diff(off), len(off) - 1, int(off[-1])
    Xd, yd = torch.from_numpy(X).cuda(), torch.from_numpy(y).cuda()
    exact = mode == "fp64"
    Ds = [N.Design(X[a:b], fi, center, scale, "wide" if wide else "fused")
          for a, b in zip(off[:-1], off[1:])]
    prev = None
    for m in N.ITERS:
        fit = _dense_fit(M, fam)(Xd, yd, off, fit_intercept=fi, center=center, scale=scale,
                                 hessian=mode, max_iter=m, rows_per_chunk=N.RPC)
        tag = f"{N.case_id(case)} max_iter={m}"
        iters, status, p32, rows32, p64 = _expected_passes(ys, m, nk)
        st = fit.stats
        print(tag, "stats", {k: st[k] for k in ("iterations", "passes_fp32", "rows_fp32",
                                                "passes_fp64", "passes_f32x",
                                                "polish_partitions")})
        # max_iter full-data iterations from the start point, no warm-start level
        assert st["iterations"] == max(iters)
        assert st["passes_fp32"] == p32 and st["rows_fp32"] == rows32
        if not exact and all(s == MAXITER for s in status) and p64 == 0:
            assert st["rows_fp32"] == st["passes_fp32"] * n
        assert st["passes_f32x"] == 0
        n_polish = sum(s == MAXITER for s in status)
        assert st["polish_partitions"] == n_polish
        assert st["passes_fp64"] == p64 + (1 if n_polish else 0)
        assert fit.iters.cpu().numpy().tolist() == iters
        assert fit.status.cpu().numpy().tolist() == status
        th = fit.theta.cpu().numpy()
        for k in range(K):
            a, b = off[k], off[k + 1]
            took_step = m <= len(ys[k][0]) and prev is not None
            e = ys[k][0][min(m, len(ys[k][0])) - 1]
            _check_iterate(f"{tag} k={k}", th[k], e, exact,
                           (Ds[k], y[a:b], fam, prev[k]) if took_step else None)
        prev = th
        if fam == "poisson":  # the budget is spent: the polish publishes at the returned theta
            _check_outputs_at_theta(tag, fit, fam, X, y, off, fi, center, scale)


@pytest.mark.parametrize("case", N.FUSED_CASES, ids=N.case_id)
def test_iterates_fused(torch_cuda, M, case):
    """NT 1-12 of the cooperative pass, both sides of P = 112 / 128, bf16 /
    fp32 / fp64 Hessians, logistic and Poisson; theta_1 (constant weights),
    theta_2 and theta_3 (the weights in Z)."""
    _run_case(torch_cuda, M, case, False)


@pytest.mark.parametrize("case", N.WIDE_CASES, ids=N.case_id)
def test_iterates_wide(torch_cuda, M, case):
    """The wide fused bf16 pass (both PP tiers) and the exact Gram."""
    _run_case(torch_cuda, M, case, True)


def test_iterates_categorical(torch_cuda, M):
    """Every pass of the categorical path is exact: the fp64 tolerance."""
    torch = torch_cuda
    Xn, codes, y, levels, off, Xd = N.cat_data()
    trs = [N.step_yardsticks(N.Design(Xd[a:b], True), y[a:b], "logistic", True, "fp64",
                             max(N.CAT_ITERS), N.RPC) for a, b in zip(off[:-1], off[1:])]
    for m in N.CAT_ITERS:
        fit = M.logistic_model_batched_categorical(
            torch.from_numpy(Xn).cuda(), torch.from_numpy(codes).cuda(), torch.from_numpy(y).cuda(),
            off, levels, fit_intercept=True, max_iter=m, rows_per_chunk=N.RPC)
        assert fit.stats["iterations"] == m
        assert fit.iters.cpu().numpy().tolist() == [m] * 3
        assert fit.status.cpu().numpy().tolist() == [MAXITER] * 3
        th = fit.theta.cpu().numpy()
        for k in range(3):
            _check_iterate(f"categorical max_iter={m} k={k}", th[k], trs[k][0][m - 1], True)
        _check_outputs_at_theta(f"categorical max_iter={m}", fit, "logistic", Xd, y, off, True,
                                None, None)


@pytest.mark.parametrize("mode", ["mixed", "fp64"])
def test_halving_accounting(torch_cuda, M, mode):
    """The overshoot case (start theta = 0, mean y ~ 39): theta_1 = theta_0 +
    d, then theta_0 + d / 2, d / 4, d / 8 -- a halving consumes an iteration
    and takes no new step -- then the next Newton step."""
    torch = torch_cuda
    X, y, off = N.halving_data()
    K, nk = len(off) - 1, np.diff(off)
    Xd, yd = torch.from_numpy(X).cuda(), torch.from_numpy(y).cuda()
    ys = [N.step_yardsticks(N.Design(X[a:b]), y[a:b], "poisson", False, mode,
                            max(N.HALVING_ITERS), N.RPC) for a, b in zip(off[:-1], off[1:])]
    Ds = [N.Design(X[a:b]) for a, b in zip(off[:-1], off[1:])]
    th1 = prev = None
    for m in N.HALVING_ITERS:
        fit = M.poisson_model_batched(Xd, yd, off, hessian=mode, max_iter=m,
                                      rows_per_chunk=N.RPC)
        tag = f"halving {mode} max_iter={m}"
        iters, status, p32, rows32, p64 = _expected_passes(ys, m, nk)
        assert fit.stats["iterations"] == m
        assert fit.stats["passes_fp32"] == p32 and fit.stats["rows_fp32"] == rows32
        assert fit.stats["passes_f32x"] == 0
        assert fit.iters.cpu().numpy().tolist() == [m] * K
        assert fit.status.cpu().numpy().tolist() == [MAXITER] * K
        th = fit.theta.cpu().numpy()
        if m == 1:
            th1 = th.copy()
        for k in range(K):
            e = ys[k][0][m - 1]
            _check_iterate(f"{tag} k={k} halved={e['rec']['halved']}", th[k], e, mode == "fp64",
                           (Ds[k], y[off[k]:off[k + 1]], "poisson", prev[k]) if m > 1 else None)
            if e["rec"]["halved"]:  # theta_0 = 0: exactly the first step, scaled
                assert np.array_equal(th[k], th1[k] * 2.0 ** -e["rec"]["bt"]), (tag, k)
        prev = th
        _check_outputs_at_theta(tag, fit, "poisson", X, y, off, False, None, None)


@pytest.mark.parametrize("case,seed,tol,switch_tol", N.CONVERGED,
                         ids=[N.case_id(c[0]) for c in N.CONVERGED])
def test_no_escalation_on_a_clean_design(torch_cuda, M, case, seed, tol, switch_tol):
    """To convergence at the small sizes: the bf16 steps contract at ~4e-4 per
    iteration, nowhere near the stall rule's 0.5, so no fp32 escalation pass
    runs and the exact passes are the emulator's.  A pass that lost part of H
    contracts slower and trips the rule."""
    torch = torch_cuda
    fam, mode, p, fi, std = case
    X, y, off, center, scale = N.case_data(fam, p, fi, std, False, seed)
    trs = [N.trajectory(X[a:b], y[a:b], fam, fi, center, scale, mode=mode, max_iter=100, tol=tol,
                        switch_tol=switch_tol) for a, b in zip(off[:-1], off[1:])]
    fit = _dense_fit(M, fam)(torch.from_numpy(X).cuda(), torch.from_numpy(y).cuda(), off,
                             fit_intercept=fi, hessian=mode, tol=tol, switch_tol=switch_tol,
                             rows_per_chunk=N.RPC)
    st = fit.stats
    emu_iters = [tr["iters"] for tr in trs]
    exact_its = set()
    for tr in trs:
        exact_its |= set(N.exact_iterations(tr))
    print(N.case_id(case), "iters", fit.iters.cpu().numpy().tolist(), "emulator", emu_iters,
          "passes_fp64", st["passes_fp64"], "emulator", len(exact_its), "passes_f32x",
          st["passes_f32x"], "passes_fp32", st["passes_fp32"])
    assert fit.status.cpu().numpy().tolist() == [OK] * len(trs)
    assert st["passes_f32x"] == 0
    assert st["passes_fp64"] == len(exact_its)
    assert (fit.iters.cpu().numpy() <= np.asarray(emu_iters) + 1).all()
    for k, tr in enumerate(trs):
        assert _rel(fit.theta[k].cpu(), tr["final"]) < REL


def test_many_partitions_poisson(torch_cuda, M):
    """K = 300 > 256: the 256-thread solve kernel and the partial sums with the
    constant-term slab (three chunks per partition), converged and through the
    polish after max_iter = 2."""
    torch = torch_cuda
    X, y, off = N.many_data()
    Xd, yd = torch.from_numpy(X).cuda(), torch.from_numpy(y).cuda()
    K = N.MANY_K
    fit = M.poisson_model_batched(Xd, yd, off, fit_intercept=True, rows_per_chunk=N.MANY_RPC)
    assert fit.stats["n_chunks"] == 3 * K
    assert fit.status.cpu().numpy().tolist() == [OK] * K
    for k in N.MANY_SAMPLE:
        a, b = off[k], off[k + 1]
        ref = G.fit("poisson", X[a:b], y[a:b], fit_intercept=True)
        e = (_rel(fit.theta[k].cpu(), ref["theta"]), _rel(fit.sig_inv[k].cpu(), ref["sig_inv"]),
             _rel(fit.sig_inv_theta[k].cpu(), ref["sig_inv_theta"]),
             abs(float(fit.loglik[k]) - ref["loglik"]) / abs(ref["loglik"]))
        print(f"K=300 converged k={k} theta {e[0]:.2e} sig_inv {e[1]:.2e} sig_inv_theta "
              f"{e[2]:.2e} loglik {e[3]:.2e}")
        assert e[0] < REL and e[1] < REL and e[2] < REL and e[3] < REL_LL

    th1 = M.poisson_model_batched(Xd, yd, off, fit_intercept=True, max_iter=1,
                                  rows_per_chunk=N.MANY_RPC).theta.cpu().numpy()
    fit = M.poisson_model_batched(Xd, yd, off, fit_intercept=True, max_iter=2,
                                  rows_per_chunk=N.MANY_RPC)
    assert fit.stats["iterations"] == 2 and fit.stats["polish_partitions"] == K
    assert fit.stats["passes_fp32"] == 2 and fit.stats["rows_fp32"] == 2 * int(off[-1])
    assert fit.iters.cpu().numpy().tolist() == [2] * K
    assert fit.status.cpu().numpy().tolist() == [MAXITER] * K
    th = fit.theta.cpu().numpy()
    for k in N.MANY_SAMPLE:
        a, b = off[k], off[k + 1]
        D = N.Design(X[a:b], True)
        steps, _ = N.step_yardsticks(D, y[a:b], "poisson", True, "mixed", 2, N.MANY_RPC)
        _check_iterate(f"K=300 max_iter=1 k={k}", th1[k], steps[0], False)
        _check_iterate(f"K=300 max_iter=2 k={k}", th[k], steps[1], False,
                       (D, y[a:b], "poisson", th1[k]))
    _check_outputs_at_theta("K=300 max_iter=2", fit, "poisson", X, y, off, True, None, None,
                            parts=N.MANY_SAMPLE)
