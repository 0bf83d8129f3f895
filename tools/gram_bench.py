#!/usr/bin/env python3
"""Timing of the score outer-product pass (dlsa_glm_gram_batched, the meat of
the sandwich covariance) through the C-ABI, against the fit's fp64 exact pass
on the same data in the same process:

  logistic        kind = score at each partition's own theta, no row extras
  poisson_both    the Poisson family with an offset and prior weights (16 more
                  bytes per row)
  irls_wave_fp64  the per-wave fp64 pass of the fit (irls_wave_kernel): a
                  dlsa_logistic_fit_batched_ex run in DLSA_HESSIAN_FP64 mode
                  without warm-start levels, whose every pass is that kernel
                  over all rows; its time per pass from dlsa_last_fit_stats

    python tools/gram_bench.py [--n 10000000] [--p 100] [--rows 97656] [--rounds 9]
        [--out profiles/gram_bench.json]

p columns and an intercept, partitions of about --rows rows.  Each call is
timed with device events on the calling stream (the entry synchronises it
before it returns: the reductions of the chunk partials are inside) after
--warmup untimed calls; a leg reports the median over --rounds calls, ns per
row, the algorithmic bytes per row and that traffic as a fraction of 8 TB/s.
``ratio_vs_irls_wave`` is a leg's time per row over the fp64 pass's.  Prints
one JSON line and writes it to --out.  Needs the GPU: no fallback.
"""

import argparse
import ctypes
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_BYTES_PER_S = 8.0e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=10_000_000)
    ap.add_argument("--p", type=int, default=100)
    ap.add_argument("--rows", type=int, default=97_656, help="rows per partition, about")
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--fit-iters", type=int, default=6, help="passes of the reference fit")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gram_bench.json"))
    args = ap.parse_args()

    import numpy as np
    import torch

    from dlsa_amd import _hip
    from dlsa_amd import models as M

    dev = M._require_gpu()
    lib = _hip.load()
    n, p = args.n, args.p
    P = p + 1
    K = max(1, round(n / args.rows))
    off = (np.arange(K + 1, dtype=np.int64) * n) // K
    off_p = off.ctypes.data_as(ctypes.c_void_p)
    stream = M._stream(dev)
    f64 = dict(dtype=torch.float64, device=dev)

    X, y = M.simulate_logistic_device(n, p, seed=2019)
    g = torch.Generator(device="cpu").manual_seed(7)
    thetas = (torch.randn((K, P), generator=g, dtype=torch.float64) * 0.3).to(dev)
    o = torch.empty(n, **f64).uniform_(float(np.log(0.2)), float(np.log(5.0)))
    w = torch.empty(n, **f64).uniform_(0.2, 5.0)
    gram, score = torch.empty((K, P, P), **f64), torch.empty((K, P), **f64)
    gsum, ssum = torch.empty((P, P), **f64), torch.empty((P,), **f64)

    def timed(family, od, wd):
        row_bytes = 8 * p + 8 + 8 * ((od is not None) + (wd is not None))
        ms = []
        for r in range(args.warmup + args.rounds):
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            _hip.check(lib.dlsa_glm_gram_batched(
                family, _hip.GRAM_SCORE, M._ptr(X), M._ptr(y), M._ptr(od), M._ptr(wd), off_p, K, p,
                1, None, None, M._ptr(thetas), P, M._ptr(gram), M._ptr(score), M._ptr(gsum),
                M._ptr(ssum), stream), "score pass")
            t1.record()
            t1.synchronize()
            if r >= args.warmup:
                ms.append(t0.elapsed_time(t1))
        med = statistics.median(ms)
        assert bool(torch.isfinite(gsum).all()) and bool(torch.isfinite(ssum).all())
        return {"ms": med, "ms_min": min(ms), "ms_max": max(ms), "ns_per_row": med * 1e6 / n,
                "bytes_per_row": row_bytes,
                "fraction_of_8TBps": n * row_bytes / (med * 1e-3) / HBM_BYTES_PER_S}

    legs = {"logistic": timed(_hip.FAMILY_LOGISTIC, None, None),
            "poisson_both": timed(_hip.FAMILY_POISSON, o, w)}
    del o, w, gram

    # the fit's fp64 pass on the same rows
    th, sig, sigt, ll, it, st = M._alloc_outputs(K, P, dev)
    per_pass = []
    for r in range(3):
        opt = _hip.default_options()
        opt.hessian_mode = _hip.HESSIAN_FP64
        opt.exact_pass = _hip.EXACT_FP64
        opt.record_timing = 1
        opt.warm_start = 0
        _hip.check(lib.dlsa_logistic_fit_batched_ex(
            M._ptr(X), M._ptr(y), off_p, K, p, 1, None, None, args.fit_iters, 1e-10, M._ptr(th),
            M._ptr(sig), M._ptr(sigt), M._ptr(ll), M._ptr(it), M._ptr(st), ctypes.byref(opt),
            stream), "reference fit")
        s = _hip.last_fit_stats()
        assert s["passes_fp64"] > 0 and s["passes_fp32"] == 0 and s["passes_oz"] == 0, s
        assert s["rows_fp64"] == s["passes_fp64"] * n, s
        per_pass.append(s["ms_pass_fp64"] / s["passes_fp64"])
    ref = statistics.median(per_pass)
    legs["irls_wave_fp64"] = {"ms": ref, "ms_min": min(per_pass), "ms_max": max(per_pass),
                              "ns_per_row": ref * 1e6 / n, "bytes_per_row": 8 * p + 8,
                              "fraction_of_8TBps": n * (8 * p + 8) / (ref * 1e-3) / HBM_BYTES_PER_S}
    res = {"lib": os.environ.get("DLSA_LIB", "in-tree"), "n": n, "p": p, "P": P, "K": K,
           "rounds": args.rounds, "legs": legs,
           "ratio_vs_irls_wave": {k: legs[k]["ms"] / ref for k in ("logistic", "poisson_both")},
           "device": torch.cuda.get_device_name(dev)}
    line = json.dumps(res)
    print(line, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
