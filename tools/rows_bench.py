#!/usr/bin/env python3
"""Timing of the row diagnostics pass (dlsa_glm_rows_batched: eta, mu, the two
residuals and the leverage of every row) through the C-ABI, against the score
pass's information matrix (dlsa_glm_gram_batched, kind = information) on the
same rows in the same process, the two alternating:

  logistic        each partition at its own theta and factor, no row extras
  poisson_both    the Poisson family with an offset and prior weights (16 more
                  bytes per row)

    python tools/rows_bench.py [--n 10000000] [--p 100] [--rows 97656] [--rounds 9]
        [--out profiles/rows_bench.json]

p columns and an intercept, partitions of about --rows rows.  Each call is
timed with device events on the calling stream (the entries synchronise it
before they return) after --warmup untimed calls of both; a leg reports the
median over --rounds calls of the rows pass (``rows``) and of the gram pass
(``gram``), the algorithmic bytes per row and ``ratio`` = rows / gram.  The
factors R_k come from the gram pass's own information matrices
(``models.rows_factor``, on the host, outside the timed calls).

A second line gives the end-to-end cost of ``dlsa_fit_sharded(cov_type="HC3")``
over ``cov_type="HC0"`` on the logistic data: host wall time of each call
(fits, passes, the host factorisation, the tail), alternating, the median of
--e2e-rounds.  Prints both JSON lines and writes them to --out.  Needs the
GPU: no fallback.
"""

import argparse
import ctypes
import json
import os
import statistics
import sys
import time

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
    ap.add_argument("--e2e-rounds", type=int, default=3, help="0: no end-to-end line")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rows_bench.json"))
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
    outs = [torch.empty(n, **f64) for _ in range(5)]

    def gram_call(family, od, wd):
        _hip.check(lib.dlsa_glm_gram_batched(
            family, _hip.GRAM_INFORMATION, M._ptr(X), M._ptr(y), M._ptr(od), M._ptr(wd), off_p, K,
            p, 1, None, None, M._ptr(thetas), P, M._ptr(gram), M._ptr(score), None, None, stream),
            "gram pass")

    def rows_call(family, od, wd, R):
        _hip.check(lib.dlsa_glm_rows_batched(
            family, M._ptr(X), M._ptr(y), M._ptr(od), M._ptr(wd), off_p, K, p, 1, None, None,
            M._ptr(thetas), P, M._ptr(R), P * P, *[M._ptr(t) for t in outs], stream), "rows pass")

    def event_ms(fn):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        fn()
        t1.record()
        t1.synchronize()
        return t0.elapsed_time(t1)

    def stats(ms, row_bytes):
        med = statistics.median(ms)
        return {"ms": med, "ms_min": min(ms), "ms_max": max(ms), "ns_per_row": med * 1e6 / n,
                "bytes_per_row": row_bytes,
                "fraction_of_8TBps": n * row_bytes / (med * 1e-3) / HBM_BYTES_PER_S}

    def leg(family, od, wd):
        read = 8 * p + 8 + 8 * ((od is not None) + (wd is not None))
        gram_call(family, od, wd)
        R = M._dev_f64(M.rows_factor(gram.cpu().numpy(), K, P), dev)
        assert bool(torch.isfinite(R).all())
        ms_r, ms_g = [], []
        for r in range(args.warmup + args.rounds):  # alternating
            a = event_ms(lambda: rows_call(family, od, wd, R))
            b = event_ms(lambda: gram_call(family, od, wd))
            if r >= args.warmup:
                ms_r.append(a)
                ms_g.append(b)
        h = outs[4]
        assert all(bool(torch.isfinite(t).all()) for t in outs)
        hsum = float(h.sum()) / (K * P)  # sum h = P per partition
        assert abs(hsum - 1.0) < 1e-6, hsum
        res = {"rows": stats(ms_r, read + 40), "gram": stats(ms_g, read)}
        res["ratio"] = res["rows"]["ms"] / res["gram"]["ms"]
        return res

    legs = {"logistic": leg(_hip.FAMILY_LOGISTIC, None, None),
            "poisson_both": leg(_hip.FAMILY_POISSON, o, w)}
    res = {"lib": os.environ.get("DLSA_LIB", "in-tree"), "n": n, "p": p, "P": P, "K": K,
           "rounds": args.rounds, "legs": legs, "device": torch.cuda.get_device_name(dev)}
    lines = [json.dumps(res)]
    print(lines[0], flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(lines[0] + "\n")
    if args.e2e_rounds <= 0:
        return
    del o, w, gram, outs

    from dlsa_amd.distributed import dlsa_fit_sharded

    def wall(cov_type):
        torch.cuda.synchronize()
        t = time.perf_counter()
        out = dlsa_fit_sharded(X, y, off, fit_intercept=True, cov_type=cov_type)
        torch.cuda.synchronize()
        assert np.isfinite(out["cov"]).all()
        return (time.perf_counter() - t) * 1e3, out

    wall("HC0"), wall("HC3")  # warm-up of both
    ms = {"HC0": [], "HC3": []}
    for _ in range(args.e2e_rounds):
        for ct in ("HC0", "HC3"):
            t, out = wall(ct)
            ms[ct].append(t)
            if ct == "HC3":
                se3 = out["std_err"]
            else:
                se0 = out["std_err"]
    e2e = {"what": "dlsa_fit_sharded end to end, host wall ms", "n": n, "p": p, "K": K,
           "rounds": args.e2e_rounds,
           "HC0_ms": statistics.median(ms["HC0"]), "HC3_ms": statistics.median(ms["HC3"]),
           "std_err_ratio_max": float((se3 / se0).max())}
    e2e["HC3_over_HC0_ms"] = e2e["HC3_ms"] - e2e["HC0_ms"]
    lines.append(json.dumps(e2e))
    print(lines[1], flush=True)
    with open(args.out, "a") as f:
        f.write(lines[1] + "\n")


if __name__ == "__main__":
    main()
