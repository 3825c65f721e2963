#!/usr/bin/env python3
"""tools/ensemble_verify_bench.py — cost of the ensemble verification (csim_ensemble_verify*), one JSON line per
configuration.

For B members of n x n (Dirichlet on all sides, the same advection physics for every member) against a host truth
field (M = B forecast members), with the thresholds 0.25, 0.5, 0.75:
  verify_call_us  one synchronous csim_ensemble_verify with every output NULL (the truth's copy, the kernel, its launch
                  and one stream sync; no copy to the host), the mean over `--calls` calls, median of three regions;
  verify_gbps     the compulsory bytes 8 (B + 1 + 4) (n+2)^2 (read every member and the truth once, write the CRPS and
                  three Brier fields) over that time (the kernel's own duration comes from a rocprofv3 --kernel-trace
                  run of `--only-verify`, which also runs the quantile kernel (levels 0.1, 0.5, 0.9) on the same
                  ensembles);
  loop_ratio      `--loops` x (verify_begin(); run(20); verify_wait()) through the C ABI against `--loops` x run(20)
                  then one sync, both medians of three regions; loop_over_run_plus_verify compares the loop with
                  run(20) + verify_call_us.
Before timing, every output for the uploaded fields is checked against the numpy restatement of
tests/test_gpu_ensemble_verify.py.

  python tools/ensemble_verify_bench.py --config 256x256 --config 64x512 --config 64x1024 [--out F]
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
sys.path.insert(0, os.path.join(ROOT, "tests"))
from __graft_entry__ import load_package  # noqa: E402
from test_gpu_ensemble_verify import restate, same  # noqa: E402

D, VX, VY = 0.05, 0.5, 0.25
RUN = 20
THRESHOLDS = [0.25, 0.5, 0.75]
LEVELS = [0.1, 0.5, 0.9]


def timed(fn, regions=3):
    out = []
    for _ in range(regions):
        t0 = time.perf_counter()
        fn()
        out.append(time.perf_counter() - t0)
    return statistics.median(out)


def matches_numpy(got, a, y):
    crps, brier, hist, _ = restate(a, y, THRESHOLDS, False)
    return same(got.crps, crps) and same(got.brier, brier) and np.array_equal(got.rank_hist, hist)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", action="append", default=[], help="BxN: B members of N x N")
    ap.add_argument("--calls", type=int, default=20, help="verify calls per timed region")
    ap.add_argument("--loops", type=int, default=10, help="begin / run / wait iterations per timed region")
    ap.add_argument("--only-verify", action="store_true",
                    help="only --calls verify calls and as many quantile calls (for a profiler run)")
    ap.add_argument("--out", help="append the JSON lines to this file too")
    args = ap.parse_args()
    pkg = load_package()
    pkg.set_device(0)
    C = pkg.C
    dt = min(0.1, pkg.safe_dt(1.0, 1.0, VX, VY, D))
    lib = pkg.lib()
    dp = C.POINTER(C.c_double)
    ts, qs = np.array(THRESHOLDS), np.array(LEVELS)
    tp, qp = ts.ctypes.data_as(dp), qs.ctypes.data_as(dp)
    for cfg in args.config or ["256x256", "64x512", "64x1024"]:
        B, n = (int(v) for v in cfg.split("x"))
        rng = np.random.default_rng(B * 7 + n)
        e = pkg.Ensemble(B, n, n, 1.0, 1.0, [0, 0, 0, 0])
        e.upload_all(rng.random((B, n + 2, n + 2)))
        y = rng.random((n + 2, n + 2))
        yp = y.ctypes.data_as(dp)
        e.set_physics(D, dt, VX, VY)

        def call():
            for _ in range(args.calls):
                if lib.csim_ensemble_verify(e._h, yp, -1, 0, len(ts), tp, None, None, None, None):
                    raise SystemExit(lib.csim_last_error().decode())
        if args.only_verify:
            call()
            for _ in range(args.calls):
                if lib.csim_ensemble_quantiles(e._h, len(qs), qp, 0, None, None, None):
                    raise SystemExit(lib.csim_last_error().decode())
            e.close()
            continue
        a = e.download_all()
        if not matches_numpy(e.verify(y, thresholds=THRESHOLDS), a, y):
            raise SystemExit(f"{cfg}: verification differs from the numpy restatement")
        del a
        call()
        t_call = timed(call) / args.calls
        nbytes = 8 * (B + 1 + 1 + len(ts)) * (n + 2) ** 2

        def loop():  # through the C ABI: the results stay in the pinned buffers
            for _ in range(args.loops):
                if lib.csim_ensemble_verify_begin(e._h, yp, -1, 0, len(ts), tp) or \
                        lib.csim_ensemble_run(e._h, RUN) or lib.csim_ensemble_verify_wait(e._h, None, None, None, None):
                    raise SystemExit(lib.csim_last_error().decode())

        def runs():
            for _ in range(args.loops):
                e.run(RUN)
            e.sync()
        loop()
        runs()
        t_loop, t_run = timed(loop) / args.loops, timed(runs) / args.loops
        rec = dict(config=cfg, members=B, n=n, thresholds=THRESHOLDS, compulsory_bytes=nbytes, calls=args.calls,
                   verify_call_us=t_call * 1e6, verify_gbps=nbytes / t_call / 1e9, run20_us=t_run * 1e6,
                   loop_us=t_loop * 1e6, loop_ratio=t_loop / t_run, loop_over_run_plus_verify=t_loop / (t_run + t_call),
                   step_us=t_run / RUN * 1e6, verify_over_step=t_call / (t_run / RUN))
        e.close()
        line = json.dumps(rec)
        print(line, flush=True)
        if args.out:
            with open(args.out, "a") as f:
                f.write(line + "\n")


if __name__ == "__main__":
    main()
