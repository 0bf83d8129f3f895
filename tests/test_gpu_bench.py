"""bench.py as a command on the GPU: a plain run does the timed steps and
nothing else, and --dump-outputs writes what the last timed step returned."""

import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REL = 1e-8  # the suite's parity tolerance (max |diff| / max |ref|)


def _rel(a, b):
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)


def test_plain_bench_is_lean_and_dumps_last_step(tmp_path):
    """`bench.py --gpus 1 --steps 3 --warmup 1 --dump-outputs DIR` without
    --full: the line keeps its headline fields, steps is the number of timed
    steps (one stats record per step goes into the kernel figures), none of
    the --full legs ran, and DIR holds float64 arrays within 64 MB that equal
    a fit of the same inputs (same seed, generated in HBM) in this process."""
    import torch

    from dlsa_amd.dlsa import reduce_partitions_device, split_reduced, wlse
    from dlsa_amd.lsa import lars_lsa
    from dlsa_amd.models import logistic_model_batched, simulate_logistic_device

    n, p, K, seed = 1_600_000, 100, 16, 2019
    out_dir = tmp_path / "dump"
    env = {k: v for k, v in os.environ.items()
           if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--n", str(n),
           "--partitions", str(K), "--steps", "3", "--warmup", "1", "--seed", str(seed),
           "--dump-outputs", str(out_dir)]
    r = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    out = json.loads(lines[0])
    assert out["unit"] == "rows/s" and out["higher_is_better"] is True and out["dtype"] == "f64"
    assert out["steps"] == 3 and out["warmup"] == 1 and out["ms_per_step"] > 0
    assert abs(out["value"] - n / (out["ms_per_step"] * 1e-3)) <= 1e-6 * out["value"]
    assert out["roofline"]["frac"] > 0 and out["kernels"]
    for key in ("parity_rel", "sig_inv_all_partitions", "cpu_baseline", "vs_cpu_baseline",
                "sig_inv_fp64_ms_per_step", "exact_fp64_ms_per_step"):
        assert key not in out, key

    files = sorted(os.listdir(out_dir))
    assert files == sorted(f"{k}.npy" for k in (
        "theta", "sig_inv", "sig_inv_theta", "loglik", "iters", "status", "sig_inv_sum",
        "sig_inv_theta_sum", "wlse", "beta_dbic"))
    got = {f[:-4]: np.load(out_dir / f) for f in files}
    assert all(a.dtype == np.float64 for a in got.values())
    assert sum(os.path.getsize(out_dir / f) for f in files) <= 64_000_000
    assert got["theta"].shape == (K, p) and got["sig_inv"].shape == (K, p, p)
    assert (got["status"] == 0).all()

    X, y = simulate_logistic_device(n, p, seed=seed, row0=0, device=torch.device("cuda", 0))
    offsets = (np.arange(K + 1, dtype=np.int64) * n) // K
    fit = logistic_model_batched(X, y, offsets, tol=1e-10)
    for name in ("theta", "sig_inv", "sig_inv_theta", "loglik"):
        assert _rel(got[name], getattr(fit, name).cpu().numpy()) < REL, name
    assert got["iters"].shape == (K,) and (got["iters"] >= 1).all()
    S, v, _, _ = split_reduced(reduce_partitions_device(fit).cpu().numpy(), fit.P)
    assert _rel(got["sig_inv_sum"], S) < REL and _rel(got["sig_inv_theta_sum"], v) < REL
    est = wlse(S, v)
    assert _rel(got["wlse"], est) < REL
    lars = lars_lsa(S, est, False, n, type="lasso")
    beta = lars["beta"][int(np.argmin(lars["BIC"]))]
    assert np.array_equal(got["beta_dbic"] != 0, beta != 0)
    assert _rel(got["beta_dbic"], beta) < REL
