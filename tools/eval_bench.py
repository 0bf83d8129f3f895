#!/usr/bin/env python3
"""Timing of the evaluation pass (the reference's second pass over the data,
dlsa/model_eval.py:10-42) through the C-ABI, three legs:

  dense_p100              dlsa_logistic_loglik_batched_sum at a config-2-like shape (p = 100)
  codes_config3           dlsa_logistic_loglik_categorical at the config-3 shape
                          (AIRLINE_NUMERIC numeric columns + AIRLINE_FACTORS codes)
  codes_config3_weighted  dlsa_logistic_loglik_categorical_weighted on the same rows with
                          omega ~ U(0.2, 5) (8 more bytes per row); leg name "weighted"
  codes_config3_poisson   dlsa_poisson_loglik_categorical on the same rows, once per
                          row-extras mask (none, offset, weights, both: 85 to 101 bytes per
                          row), betas scaled down so that exp(eta) stays finite; leg name
                          "poisson"
  dense_expanded_config3  the dense pass on expand_categorical of the same rows: what
                          the evaluation had to read before the code-layout pass

    python tools/eval_bench.py [--n 10000000] [--K 100] [--B 4] [--rounds 9]

Each call is timed with device events on the calling stream (the entry
points synchronise it before they return) after --warmup untimed calls; a
leg reports the median over --rounds calls, rows/s, the algorithmic bytes
per row (8 p + 8 dense, 8 q + F + 8 in the code layout) and that traffic as a
fraction of 8 TB/s.  Prints one JSON line.  Needs the GPU: no fallback.
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
    ap.add_argument("--K", type=int, default=100)
    ap.add_argument("--B", type=int, default=4)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--legs", default="dense,codes,expanded",
                    help="comma-separated subset (A/B runs of one kernel across library builds)")
    args = ap.parse_args()

    import numpy as np
    import torch

    from dlsa_amd import _hip
    from dlsa_amd import models as M

    dev = M._require_gpu()
    lib = _hip.load()
    n, K, B = args.n, args.K, args.B
    off = (np.arange(K + 1, dtype=np.int64) * n) // K
    off_p = off.ctypes.data_as(ctypes.c_void_p)
    stream = M._stream(dev)

    def timed(call, row_bytes):
        out = torch.empty((K, B), dtype=torch.float64, device=dev)
        tot = torch.empty((B,), dtype=torch.float64, device=dev)
        ms = []
        for r in range(args.warmup + args.rounds):
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            _hip.check(call(out, tot), "evaluation pass")
            t1.record()
            t1.synchronize()
            if r >= args.warmup:
                ms.append(t0.elapsed_time(t1))
        med = statistics.median(ms)
        return {"ms": med, "ms_min": min(ms), "ms_max": max(ms), "rows_per_s": n / (med * 1e-3),
                "bytes_per_row": row_bytes,
                "fraction_of_8TBps": n * row_bytes / (med * 1e-3) / HBM_BYTES_PER_S}, tot.cpu().numpy()

    def dense(X, y, betas):
        p = X.shape[1]
        return timed(lambda out, tot: lib.dlsa_logistic_loglik_batched_sum(
            M._ptr(X), M._ptr(y), off_p, K, p, 1, None, None, M._ptr(betas), B, M._ptr(out),
            M._ptr(tot), stream), 8 * p + 8)

    want = set(args.legs.split(","))
    legs = {}
    res = {"lib": os.environ.get("DLSA_LIB", "in-tree"), "n": n, "K": K, "B": B,
           "rounds": args.rounds, "legs": legs, "device": None}
    g = torch.Generator(device="cpu").manual_seed(7)

    if "dense" in want:
        p = 100
        X, y = M.simulate_logistic_device(n, p, seed=2019)
        betas = (torch.randn((B, p + 1), generator=g, dtype=torch.float64) * 0.3).to(dev)
        legs["dense_p100"], _ = dense(X, y, betas)
        del X, y

    Xn, codes, y, levels = M.simulate_categorical(n, seed=2019, device=dev)
    q, F = Xn.shape[1], codes.shape[1]
    P = 1 + q + int((levels - 1).sum())
    betas = (torch.randn((B, P), generator=g, dtype=torch.float64) * 0.3).to(dev)
    lv_p = levels.ctypes.data_as(ctypes.c_void_p)
    res["P_config3"] = P
    if "codes" in want:
        legs["codes_config3"], tot_c = timed(lambda out, tot: lib.dlsa_logistic_loglik_categorical(
            M._ptr(Xn), M._ptr(codes), M._ptr(y), off_p, K, q, F, lv_p, 1, None, None,
            M._ptr(betas), B, 0, M._ptr(out), M._ptr(tot), stream), 8 * q + F + 8)
    if "weighted" in want:
        w = torch.empty(n, dtype=torch.float64, device=dev).uniform_(0.2, 5.0)
        legs["codes_config3_weighted"], _ = timed(
            lambda out, tot: lib.dlsa_logistic_loglik_categorical_weighted(
                M._ptr(Xn), M._ptr(codes), M._ptr(y), M._ptr(w), off_p, K, q, F, lv_p, 1, None,
                None, M._ptr(betas), B, 0, M._ptr(out), M._ptr(tot), stream), 8 * q + F + 16)
        del w
    if "poisson" in want:
        w = torch.empty(n, dtype=torch.float64, device=dev).uniform_(0.2, 5.0)
        o = torch.empty(n, dtype=torch.float64, device=dev).uniform_(float(np.log(0.2)),
                                                                     float(np.log(5.0)))
        bp = (0.25 * betas).contiguous()
        for name, om, wm in (("none", None, None), ("offset", o, None), ("weights", None, w),
                             ("both", o, w)):
            legs["codes_config3_poisson_" + name], _ = timed(
                lambda out, tot: lib.dlsa_poisson_loglik_categorical(
                    M._ptr(Xn), M._ptr(codes), M._ptr(y), M._ptr(om), M._ptr(wm), off_p, K, q, F,
                    lv_p, 1, None, None, M._ptr(bp), B, 0, M._ptr(out), M._ptr(tot), stream),
                8 * q + F + 8 + 8 * ((om is not None) + (wm is not None)))
        del w, o
    if "expanded" in want:
        X = M.expand_categorical(Xn, codes, levels)
        del Xn, codes
        legs["dense_expanded_config3"], tot_d = dense(X, y, betas)
    if "codes" in want and "expanded" in want:
        c, d = legs["codes_config3"], legs["dense_expanded_config3"]
        res["speedup_codes_vs_dense_expanded"] = d["ms"] / c["ms"]
        res["bytes_ratio_dense_expanded_vs_codes"] = d["bytes_per_row"] / c["bytes_per_row"]
        res["max_rel_diff_codes_vs_dense_expanded"] = float(
            np.abs(tot_c - tot_d).max() / np.abs(tot_d).max())
    res["device"] = torch.cuda.get_device_name(dev)
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
