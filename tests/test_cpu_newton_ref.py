"""The Newton emulator of tests/_newton_ref.py, pinned on the CPU, and the
conditions the cases of tests/test_gpu_newton_steps.py must meet for its
tolerance to mean something.  No GPU, plain numpy.

* In "fp64" mode the emulator run to convergence is the existing references:
  _glm_ref.fit (theta and the number of halvings) and the oracle's
  logistic fit.
* For every GPU case, partition and checked iteration m: the modelled fp32
  accumulation noise of a correct approximate pass is at most 0.01 D_m, D_m
  the distance one dropped row moves theta_m -- so the GPU tolerance 0.1 D_m
  sits a factor 10 above the rounding of a correct kernel and a factor 10
  below the smallest defect of interest.
  (The rounding a whole trajectory carries from one iteration into the bf16
  image of the next is printed as "carried": it is why the GPU file compares
  each approximate step from the fit's own previous iterate.)
* No case hangs on a coin flip: every halve / switch / stall / converge
  decision the emulator takes inside the checked iterations clears its
  threshold by a factor >= 10, in the case's mode and in "fp64" mode.
"""

import numpy as np
import pytest

import _newton_ref as N
import _glm_ref as G
import oracle as O

MARGIN = 10.0
NOISE_VS_DEFECT = 0.01


def _rel(a, b):
    return np.abs(np.asarray(a) - np.asarray(b)).max() / np.abs(b).max()


def _min_margin(tr):
    return min((v for r in tr["rec"] for v in r["margins"].values()), default=np.inf)


def _weakest(tr):
    return min(((v, r["it"], k) for r in tr["rec"] for k, v in r["margins"].items()),
               default=(np.inf, 0, ""))


# ---- the emulator is the existing references --------------------------------

def test_fp64_mode_is_poisson_ref_on_the_overshoot_case():
    X, y, _ = N.halving_data()
    ref = G.fit("poisson", X, y)
    tr = N.trajectory(X, y, "poisson", mode="fp64", max_iter=200, tol=1e-12)
    halvings = sum(r["halved"] for r in tr["rec"])
    print("halvings", halvings, ref["halvings"], "iters", tr["iters"], ref["iters"],
          "theta", _rel(tr["final"], ref["theta"]))
    assert tr["status"] == "ok"
    assert ref["halvings"] >= 3 and halvings == ref["halvings"]
    # the reference halves inside an iteration, the state machine spends one on each
    assert abs(tr["iters"] - (ref["iters"] + ref["halvings"])) <= 1
    assert _rel(tr["final"], ref["theta"]) < 1e-10


def test_fp64_mode_is_poisson_ref_on_a_plain_shape():
    X, y, off, _, _ = N.case_data("poisson", 64, True, False)
    a, b = off[1], off[2]
    ref = G.fit("poisson", X[a:b], y[a:b], fit_intercept=True)
    tr = N.trajectory(X[a:b], y[a:b], "poisson", fit_intercept=True, mode="fp64", max_iter=200,
                      tol=1e-12)
    assert tr["status"] == "ok" and ref["halvings"] == 0
    assert not any(r["halved"] for r in tr["rec"])
    assert abs(tr["iters"] - ref["iters"]) <= 1
    assert _rel(tr["final"], ref["theta"]) < 1e-10


def test_fp64_mode_is_the_oracle_logistic_fit():
    X, y = O.simulate_counter(3001, 20, seed=31)
    center, scale = X.mean(0) + 0.1, X.std(0, ddof=1) * 1.5
    ref = O.logistic_fit(X, y, fit_intercept=True, center=center, scale=scale, tol=1e-12)
    tr = N.trajectory(X, y, "logistic", fit_intercept=True, center=center, scale=scale,
                      mode="fp64", max_iter=100, tol=1e-12)
    assert tr["status"] == "ok" and ref["converged"]
    assert abs(tr["iters"] - ref["iters"]) <= 1
    assert _rel(tr["final"], ref["coef"]) < 1e-10


def test_mixed_mode_switches_and_reaches_the_same_fixed_point():
    """The approximate Hessians only steer: "mixed" and "mixed_f32" end at the
    fp64 fixed point, after a phase switch, without escalation."""
    X, y, off, _, _ = N.case_data("logistic", 33, False, False)
    Xk, yk = X[:off[1]], y[:off[1]]
    want = N.trajectory(Xk, yk, mode="fp64", max_iter=100)
    for mode in ("mixed", "mixed_f32"):
        tr = N.trajectory(Xk, yk, mode=mode, max_iter=100)
        assert tr["status"] == "ok"
        assert sum(r["switched"] for r in tr["rec"]) == 1
        assert not any(r["escalated"] for r in tr["rec"])
        assert tr["rec"][0]["hmode"] == ("bf16" if mode == "mixed" else "f32")
        assert tr["rec"][-1]["hmode"] == "fp64"
        assert _rel(tr["final"], want["final"]) < 1e-9


def test_one_row_defect_is_the_trajectory_with_one_changed_step():
    X, y, off, _, _ = N.case_data("logistic", 17, False, False)
    Xk, yk = X[:off[1]], y[:off[1]]
    clean = N.trajectory(Xk, yk, mode="mixed", max_iter=3)
    for m in (1, 2, 3):
        bad = N.one_row_defect(Xk, yk, m, mode="mixed")
        assert len(bad["theta"]) == m
        for i in range(m - 1):
            assert np.array_equal(bad["theta"][i], clean["theta"][i])
        d = np.abs(bad["theta"][m - 1] - clean["theta"][m - 1]).max()
        D = N.Design(Xk)
        st, _ = N.step_yardsticks(D, yk, "logistic", False, "mixed", m, N.RPC)
        assert d > 0 and abs(d - st[m - 1]["D"]) <= 1e-6 * d


# ---- the conditions on the GPU cases ----------------------------------------

def _check_sizes(off, P, wide):
    nk = np.diff(off)
    assert (nk <= max(2048, 64 * P)).all(), "a warm-start level would run"
    assert (nk >= 10 * P).all()
    assert (nk % 32 != 0).all()
    assert any(len(N.chunk_bounds(int(n), N.RPC)) > 1 for n in nk)


ALL = [(c, False) for c in N.FUSED_CASES] + [(c, True) for c in N.WIDE_CASES]


def test_sizes_cover_the_ragged_edges():
    tails = set()
    short = False
    for c, wide in ALL:
        _, _, off, _, _ = N.case_data(c[0], *c[2:], wide=wide)
        nk = np.diff(off)
        tails |= {int(n % 32) for n in nk}
        short |= bool((nk < N.RPC).any())
    assert any(0 < t < 8 for t in tails) and short


@pytest.mark.parametrize("case,wide", ALL, ids=[N.case_id(c) + ("-wide" if w else "")
                                                 for c, w in ALL])
def test_case_conditions(case, wide):
    fam, mode, p, fi, std = case
    X, y, off, center, scale = N.case_data(fam, p, fi, std, wide)
    _check_sizes(off, p + int(fi), wide)
    ys = N.case_yardsticks(fam, mode, p, fi, std, wide)
    for k, (steps, tr) in enumerate(ys):
        assert len(steps) == max(N.ITERS) or tr["status"] == "ok"
        for e in steps:
            r = e["rec"]
            print(f"{N.case_id(case)} k={k} m={r['it']} {r['hmode']} s {e['s']:.2e} "
                  f"budget/s {e['budget'] / e['s']:.2e} noise/s {e['noise'] / e['s']:.2e} "
                  f"D/s {e['D'] / e['s']:.2e} noise/D {e['noise'] / e['D']:.2e} "
                  f"carried/s {e['carried'] / e['s']:.2e} "
                  f"margins {r['margins']}")
            assert not r["halved"] and not r["escalated"]
            assert e["D"] > 0
            assert e["noise"] <= NOISE_VS_DEFECT * e["D"]
            assert min(r["margins"].values(), default=np.inf) >= MARGIN
        if mode != "fp64":  # the same decisions with exact Hessians
            a, b = off[k], off[k + 1]
            D = N.Design(X[a:b], fi, center, scale, "wide" if wide else "fused")
            ex = N.trajectory(D, y[a:b], fam, fi, mode="fp64", max_iter=max(N.ITERS))
            assert not any(r["halved"] for r in ex["rec"])
            assert _min_margin(ex) >= MARGIN, _weakest(ex)


def test_a_truncating_bf16_conversion_is_far_outside_the_tolerance():
    """The tolerance can tell a wrong rounding: with bf16 by truncation in
    place of round-to-nearest-even the first iterate of every partition moves
    by more than twice the tolerance 0.1 D_1 (by 0.5 .. 60 D_1)."""
    for case in (("logistic", "mixed", 17, False, False), ("poisson", "mixed", 64, True, False)):
        fam, mode, p, fi, std = case
        X, y, off, center, scale = N.case_data(fam, p, fi, std)
        ys = N.case_yardsticks(*case)
        for k, (steps, _) in enumerate(ys):
            a, b = off[k], off[k + 1]
            bad = N.trajectory(X[a:b], y[a:b], fam, fi, center, scale, mode=mode, max_iter=1,
                               _convert=N._bf16_trunc)
            dist = np.abs(bad["theta"][0] - steps[0]["theta"]).max()
            print(N.case_id(case), k, "truncation / D_1", dist / steps[0]["D"])
            assert dist > 2 * 0.1 * steps[0]["D"]


def test_categorical_case_conditions():
    _, _, y, _, off, Xd = N.cat_data()
    _check_sizes(off, Xd.shape[1] + 1, False)
    for a, b in zip(off[:-1], off[1:]):
        tr = N.trajectory(Xd[a:b], y[a:b], "logistic", True, mode="fp64", max_iter=max(N.CAT_ITERS))
        assert tr["status"] == "maxiter" and not any(r["halved"] for r in tr["rec"])
        assert _min_margin(tr) >= MARGIN, _weakest(tr)


@pytest.mark.parametrize("mode", ["mixed", "fp64"])
def test_halving_case_halves_by_a_wide_margin(mode):
    """Every partition of the overshoot case: theta_1 = d, then at least three
    iterations that halve (theta_0 + d / 2, / 4, / 8), each decided by a
    log-likelihood that fell >= 10 times below the threshold (or overflowed)."""
    X, y, off = N.halving_data()
    assert (np.diff(off) <= 2048).all()
    for a, b in zip(off[:-1], off[1:]):
        tr = N.trajectory(X[a:b], y[a:b], "poisson", mode=mode, max_iter=max(N.HALVING_ITERS))
        rec = tr["rec"]
        halved = [r["halved"] for r in rec]
        print(mode, "halved", halved, "margins", [r["margins"].get("halve") for r in rec])
        assert halved[0] is False and halved[1:4] == [True, True, True]
        d = tr["theta"][0] - tr["start"]
        for i in (1, 2, 3):
            assert np.array_equal(tr["theta"][i], tr["start"] + d * 2.0 ** -i)
            assert rec[i]["bt"] == i
        assert _min_margin(tr) >= MARGIN, _weakest(tr)


@pytest.mark.parametrize("case,seed,tol,switch_tol", N.CONVERGED,
                         ids=[N.case_id(c[0]) for c in N.CONVERGED])
def test_converged_cases_never_near_the_stall_rule(case, seed, tol, switch_tol):
    """To convergence: every decision (the ones at tol included) by a factor
    10, no halving, no escalation, and wherever the stall rule could look the
    step shrank by far more than the factor 2 it asks for."""
    fam, mode, p, fi, std = case
    X, y, off, center, scale = N.case_data(fam, p, fi, std, False, seed)
    for a, b in zip(off[:-1], off[1:]):
        for md in (mode, "fp64"):
            tr = N.trajectory(X[a:b], y[a:b], fam, fi, center, scale, mode=md, max_iter=100,
                              tol=tol, switch_tol=switch_tol)
            assert tr["status"] == "ok"
            assert not any(r["halved"] or r["escalated"] for r in tr["rec"])
            assert _min_margin(tr) >= MARGIN, _weakest(tr)
            ratios = [r["stall_ratio"] for r in tr["rec"] if "stall_ratio" in r]
            print(N.case_id(case), md, "iters", tr["iters"], "exact", N.exact_iterations(tr),
                  "stall ratios", ratios)
            assert all(q <= 0.05 for q in ratios)
            if md == mode:  # the bf16 contraction rate: far from the stall rule's 0.5
                bf = [r["dm"] for r in tr["rec"] if r["hmode"] == "bf16"]
                assert bf[-1] / bf[-2] < 0.01


def test_many_partition_case_conditions():
    X, y, off = N.many_data()
    assert N.MANY_K > 256 and 256 in N.MANY_SAMPLE and 0 in N.MANY_SAMPLE
    assert N.MANY_K - 1 in N.MANY_SAMPLE and len(N.MANY_SAMPLE) == 8
    for k in N.MANY_SAMPLE:
        a, b = off[k], off[k + 1]
        D = N.Design(X[a:b], True)
        steps, tr = N.step_yardsticks(D, y[a:b], "poisson", True, "mixed", 2, N.MANY_RPC)
        for e in steps:
            assert not e["rec"]["halved"]
            assert e["noise"] <= NOISE_VS_DEFECT * e["D"]
        assert _min_margin(tr) >= MARGIN, _weakest(tr)
        ex = N.trajectory(D, y[a:b], "poisson", True, mode="fp64", max_iter=2)
        assert _min_margin(ex) >= MARGIN, _weakest(ex)
        assert G.fit("poisson", X[a:b], y[a:b], fit_intercept=True)["halvings"] == 0
