#!/usr/bin/env python3
"""Timing of the score outer-product pass on the categorical-code layout
(dlsa_glm_gram_categorical) at config 3's shape (simulate_categorical: 9
numeric columns, 5 factors, P = 182), for both families -- the Poisson one
with an offset and prior weights -- beside, in the same process and on the
same rows, one Newton pass of the categorical fit and the categorical
goodness-of-fit pass:

  bounds_sweep  the measuring sweep: the call on a copy of the codes whose last
                row holds one invalid code, which the entry ends with
                DLSA_E_INVALID after the sweep and before the gram pass (plan
                upload, sweep, readback of the counts)
  gram_pass     NOT a kernel time: the whole call minus bounds_sweep, i.e. the
                gram-mode categorical pass together with the grid kernel, the
                reduction of the chunk partials (launch_gram_reduce) and the
                final synchronisation.  newton_pass is the pass kernel alone,
                so gram_pass / newton_pass overstates the gram kernel's cost.
  whole_call    dlsa_glm_gram_categorical, kind = score at each partition's
                own theta, device events around the call
  newton_pass   the categorical fit's pass by tools/cat_pass_bench.py's method:
                fits with max_iter = 1 (one Newton pass and the polish pass),
                ms_pass_fp64 / passes_fp64 of dlsa_last_fit_stats
  gof_pass      glm_gof_batched_categorical at the same thetas (whole call)

    python tools/cat_gram_bench.py [--n 10000000] [--K 10] [--rounds 7]
        [--out profiles/cat_gram_bench.json]

Each leg is the median over --rounds calls after --warmup untimed ones.
``ratio``: gram_pass / newton_pass (an upper bound on the kernels' ratio, see
above) and bounds_sweep / gof_pass (both whole calls).  ``notes`` in the JSON
repeats what each leg includes.  Prints one
JSON line and writes it to --out.  Needs the GPU: no fallback.
"""

import argparse
import ctypes
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=10_000_000)
    ap.add_argument("--K", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cat_gram_bench.json"))
    args = ap.parse_args()

    import numpy as np
    import torch

    from dlsa_amd import _hip
    from dlsa_amd import models as M

    dev = M._require_gpu()
    lib = _hip.load()
    n, K = args.n, args.K
    Xn, codes, y01, levels = M.simulate_categorical(n, seed=2019, device=dev)
    q, F = Xn.shape[1], codes.shape[1]
    P = 1 + q + int((levels - 1).sum())
    off = (np.arange(K + 1, dtype=np.int64) * n) // K
    off_p = off.ctypes.data_as(ctypes.c_void_p)
    lv_p = levels.ctypes.data_as(ctypes.c_void_p)
    stream = M._stream(dev)
    f64 = dict(dtype=torch.float64, device=dev)
    g = torch.Generator(device=dev).manual_seed(12)
    ypois = torch.poisson(2.0 * y01 + 0.5, generator=g)
    o = torch.empty(n, **f64).uniform_(float(np.log(0.2)), float(np.log(5.0)), generator=g)
    w = torch.empty(n, **f64).uniform_(0.2, 5.0, generator=g)
    w[torch.randint(0, n, (n // 50,), generator=g, device=dev)] = 0.0
    bad_codes = codes.clone()
    bad_codes[n - 1, 0] = int(levels[0])  # ends the call after the sweep
    gram, score = torch.empty((K, P, P), **f64), torch.empty((K, P), **f64)

    def median_ms(fn):
        ms = []
        for r in range(args.warmup + args.rounds):
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            fn()
            t1.record()
            t1.synchronize()
            if r >= args.warmup:
                ms.append(t0.elapsed_time(t1))
        return {"ms": statistics.median(ms), "ms_min": min(ms), "ms_max": max(ms)}

    legs = {}
    for family, fam, y, od, wd in (("logistic", _hip.FAMILY_LOGISTIC, y01, None, None),
                                   ("poisson_both", _hip.FAMILY_POISSON, ypois, o, w)):
        # the thetas of a one-pass fit: a point with realistic eta
        if od is None:
            fit = M.logistic_model_batched_categorical(Xn, codes, y, off, levels,
                                                       fit_intercept=True, max_iter=3)
        else:
            fit = M.poisson_model_batched_categorical(Xn, codes, y, off, levels, wd,
                                                      eta_offset=od, fit_intercept=True,
                                                      max_iter=3)
        thetas = fit.theta.contiguous()
        row_bytes = 8 * q + F + 8 + 8 * ((od is not None) + (wd is not None))

        def entry(cd, want):
            rc = lib.dlsa_glm_gram_categorical(
                fam, _hip.GRAM_SCORE, M._ptr(Xn), M._ptr(cd), M._ptr(y), M._ptr(od), M._ptr(wd),
                off_p, K, q, F, lv_p, 1, None, None, M._ptr(thetas), P, 0, M._ptr(gram),
                M._ptr(score), None, None, stream)
            assert rc == want, (rc, _hip.last_error())

        whole = median_ms(lambda: entry(codes, 0))
        assert bool(torch.isfinite(gram).all()) and bool(torch.isfinite(score).all())
        sweep = median_ms(lambda: entry(bad_codes, -1))
        per = []
        for r in range(args.rounds + 1):
            if od is None:
                f1 = M.logistic_model_batched_categorical(Xn, codes, y, off, levels,
                                                          fit_intercept=True, max_iter=1,
                                                          record_timing=True)
            else:
                f1 = M.poisson_model_batched_categorical(Xn, codes, y, off, levels, wd,
                                                         eta_offset=od, fit_intercept=True,
                                                         max_iter=1, record_timing=True)
            if r:  # the first fit warms up
                per.append(f1.stats["ms_pass_fp64"] / f1.stats["passes_fp64"])
            del f1
        newton = {"ms": statistics.median(per), "ms_min": min(per), "ms_max": max(per)}
        fam_name = "logistic" if od is None else "poisson"
        gof = median_ms(lambda: M.glm_gof_batched_categorical(
            fam_name, Xn, codes, y, off, levels, thetas=thetas, eta_offset=od, sample_weight=wd,
            fit_intercept=True))
        gp = whole["ms"] - sweep["ms"]
        legs[family] = {
            "bytes_per_row": row_bytes, "bounds_sweep": sweep, "gram_pass": {"ms": gp},
            "whole_call": whole, "newton_pass": newton, "gof_pass": gof,
            "ratio": {"gram_pass_vs_newton_pass": gp / newton["ms"],
                      "bounds_sweep_vs_gof_pass": sweep["ms"] / gof["ms"]}}
        del fit
    notes = {
        "bounds_sweep": "whole call ended after the sweep by one invalid code: plan upload, "
                        "sweep kernel, readback of the counts, synchronisation",
        "gram_pass": "whole_call - bounds_sweep: gram-mode pass kernel + grid kernel + "
                     "launch_gram_reduce + synchronisation; not a kernel time",
        "whole_call": "dlsa_glm_gram_categorical, device events around the call",
        "newton_pass": "kernel only: ms_pass_fp64 / passes_fp64 of fits with max_iter = 1",
        "gof_pass": "whole call of glm_gof_batched_categorical at the same thetas",
        "gram_pass_vs_newton_pass": "an upper bound on the kernels' ratio (call overheads on "
                                    "the gram side only)"}
    res = {"lib": os.environ.get("DLSA_LIB", "in-tree"), "n": n, "K": K, "P": P, "q": q, "F": F,
           "rounds": args.rounds, "legs": legs, "notes": notes,
           "device": torch.cuda.get_device_name(dev)}
    line = json.dumps(res)
    print(line, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
