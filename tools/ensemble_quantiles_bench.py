#!/usr/bin/env python3
"""tools/ensemble_quantiles_bench.py — cost of the per-cell ensemble quantiles (csim_ensemble_quantiles*), one JSON
line per configuration.

For B members of n x n (Dirichlet on all sides, the same advection physics for every member), with the levels
0.1, 0.5, 0.9 and the thresholds 0.25, 0.75:
  quant_call_us  one synchronous csim_ensemble_quantiles with both outputs NULL (the kernel, its launch and one stream
                 sync; no copy to the host), the mean over `--calls` calls, median of three timed regions;
  quant_gbps     the compulsory bytes 8 (B + 5) (n+2)^2 (read every member once, write five fields) over that time
                 (the kernel's own duration comes from a rocprofv3 --kernel-trace run of `--only-quantiles`);
  loop_ratio     `--loops` x (quantiles_begin(); run(20); quantiles_wait()) through the C ABI against `--loops` x
                 run(20) then one sync, both medians of three regions; loop_over_run_plus_quant compares the loop with
                 run(20) + quant_call_us.
Before timing, the result for the uploaded fields is checked against np.quantile / np.mean(a > t).

  python tools/ensemble_quantiles_bench.py --config 256x256 --config 64x512 --config 64x1024 --config 16x1024 [--out F]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from __graft_entry__ import load_package  # noqa: E402

D, VX, VY = 0.05, 0.5, 0.25
RUN = 20
LEVELS = [0.1, 0.5, 0.9]
THRESHOLDS = [0.25, 0.75]


def timed(fn, regions=3):
    out = []
    for _ in range(regions):
        t0 = time.perf_counter()
        fn()
        out.append(time.perf_counter() - t0)
    return statistics.median(out)


def matches_numpy(got, a):
    for k, q in enumerate(LEVELS):
        want = np.quantile(a, q, axis=0)
        nz = want != 0
        if not (np.array_equal(got.q[k], want) and np.array_equal(got.q[k][nz].view(np.int64), want[nz].view(np.int64))):
            return False
    return all(np.array_equal(got.exceed[k], np.mean(a > t, axis=0)) for k, t in enumerate(THRESHOLDS))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", action="append", default=[], help="BxN: B members of N x N")
    ap.add_argument("--calls", type=int, default=20, help="quantile calls per timed region")
    ap.add_argument("--loops", type=int, default=10, help="begin / run / wait iterations per timed region")
    ap.add_argument("--only-quantiles", action="store_true",
                    help="only --calls quantile calls and as many statistics calls (for a profiler run)")
    ap.add_argument("--out", help="append the JSON lines to this file too")
    args = ap.parse_args()
    pkg = load_package()
    pkg.set_device(0)
    C = pkg.C
    dt = min(0.1, pkg.safe_dt(1.0, 1.0, VX, VY, D))
    lib = pkg.lib()
    qs = np.array(LEVELS)
    ts = np.array(THRESHOLDS)
    qp, tp = qs.ctypes.data_as(C.POINTER(C.c_double)), ts.ctypes.data_as(C.POINTER(C.c_double))
    for cfg in args.config or ["256x256", "64x512", "64x1024", "16x1024"]:
        B, n = (int(v) for v in cfg.split("x"))
        e = pkg.Ensemble(B, n, n, 1.0, 1.0, [0, 0, 0, 0])
        e.upload_all(np.random.default_rng(B * 7 + n).random((B, n + 2, n + 2)))
        e.set_physics(D, dt, VX, VY)

        def call():
            for _ in range(args.calls):
                if lib.csim_ensemble_quantiles(e._h, len(qs), qp, len(ts), tp, None, None):
                    raise SystemExit(lib.csim_last_error().decode())
        if args.only_quantiles:  # the statistics kernel on the same ensemble, for the ratio of kernel times
            call()
            for _ in range(args.calls):
                if lib.csim_ensemble_stats(e._h, 1, None, None, None, None):
                    raise SystemExit(lib.csim_last_error().decode())
            e.close()
            continue
        a = e.download_all()
        if not matches_numpy(e.quantiles(LEVELS, THRESHOLDS), a):
            raise SystemExit(f"{cfg}: quantiles differ from numpy")
        del a
        call()
        t_call = timed(call) / args.calls
        nbytes = 8 * (B + len(qs) + len(ts)) * (n + 2) ** 2

        def loop():  # through the C ABI: the results stay in the pinned buffers
            for _ in range(args.loops):
                if lib.csim_ensemble_quantiles_begin(e._h, len(qs), qp, len(ts), tp) or \
                        lib.csim_ensemble_run(e._h, RUN) or lib.csim_ensemble_quantiles_wait(e._h, None, None):
                    raise SystemExit(lib.csim_last_error().decode())

        def runs():
            for _ in range(args.loops):
                e.run(RUN)
            e.sync()
        loop()
        runs()
        t_loop, t_run = timed(loop) / args.loops, timed(runs) / args.loops
        rec = dict(config=cfg, members=B, n=n, levels=LEVELS, thresholds=THRESHOLDS, compulsory_bytes=nbytes,
                   calls=args.calls, quant_call_us=t_call * 1e6, quant_gbps=nbytes / t_call / 1e9,
                   run20_us=t_run * 1e6, loop_us=t_loop * 1e6, loop_ratio=t_loop / t_run,
                   loop_over_run_plus_quant=t_loop / (t_run + t_call), step_us=t_run / RUN * 1e6,
                   quant_over_step=t_call / (t_run / RUN))
        e.close()
        line = json.dumps(rec)
        print(line, flush=True)
        if args.out:
            with open(args.out, "a") as f:
                f.write(line + "\n")


if __name__ == "__main__":
    main()
