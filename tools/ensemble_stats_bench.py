#!/usr/bin/env python3
"""tools/ensemble_stats_bench.py — cost of the per-cell ensemble statistics (csim_ensemble_stats*), one JSON line per
configuration.

For B members of n x n (Dirichlet on all sides, the same advection physics for every member):
  stats_call_us  one synchronous csim_ensemble_stats with every output NULL (the kernel, its launch and one stream
                 sync; no copy to the host), the mean over `--calls` calls, median of three timed regions;
  stats_gbps     the compulsory bytes 8 (B + 4) (n+2)^2 (read every member once, write four fields) over that time
                 (a lower bound of the kernel's rate: the call's launch and sync are included — the kernel's own
                 duration comes from a rocprofv3 --kernel-trace run of `--only-stats`);
  loop_ratio     `--loops` x (stats_begin(); run(20); stats_wait()) through the C ABI against `--loops` x run(20) then
                 one sync, both medians of three regions; loop_over_run_plus_stats compares the loop with run(20) +
                 stats_call_us; loop_python_us is the same loop through Ensemble, whose stats_wait() also copies the
                 four fields into new numpy arrays.
Before timing, the statistics of the uploaded fields are checked against numpy bit for bit.

  python tools/ensemble_stats_bench.py --config 256x256 --config 64x512 --config 64x1024 [--out FILE]
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


def timed(fn, regions=3):
    out = []
    for _ in range(regions):
        t0 = time.perf_counter()
        fn()
        out.append(time.perf_counter() - t0)
    return statistics.median(out)


def same_bits(a, b):
    return np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(a[~np.isnan(b)].view(np.int64),
                                                                        b[~np.isnan(b)].view(np.int64))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", action="append", default=[], help="BxN: B members of N x N")
    ap.add_argument("--calls", type=int, default=50, help="statistics calls per timed region")
    ap.add_argument("--loops", type=int, default=20, help="begin / run / wait iterations per timed region")
    ap.add_argument("--only-stats", action="store_true", help="only --calls statistics calls (for a profiler run)")
    ap.add_argument("--calibrate", action="store_true",
                    help="with --only-stats: as many csim_ensemble_minmax calls too (one known read of every member, "
                         "to calibrate FETCH_SIZE on this layout)")
    ap.add_argument("--out", help="append the JSON lines to this file too")
    args = ap.parse_args()
    pkg = load_package()
    pkg.set_device(0)
    dt = min(0.1, pkg.safe_dt(1.0, 1.0, VX, VY, D))
    lib = pkg.lib()
    for cfg in args.config or ["256x256", "64x512", "64x1024"]:
        B, n = (int(v) for v in cfg.split("x"))
        e = pkg.Ensemble(B, n, n, 1.0, 1.0, [0, 0, 0, 0])
        e.upload_all(np.random.default_rng(B * 7 + n).random((B, n + 2, n + 2)))
        e.set_physics(D, dt, VX, VY)

        def call():
            for _ in range(args.calls):
                if lib.csim_ensemble_stats(e._h, 1, None, None, None, None):
                    raise SystemExit(lib.csim_last_error().decode())
        if args.only_stats:
            call()
            mm = np.empty((B, 2))
            for _ in range(args.calls if args.calibrate else 0):
                if lib.csim_ensemble_minmax(e._h, mm.ctypes.data_as(pkg.C.POINTER(pkg.C.c_double))):
                    raise SystemExit(lib.csim_last_error().decode())
            e.close()
            continue
        a = e.download_all()
        got = e.stats(1)
        if not (same_bits(got.mean, np.mean(a, axis=0)) and same_bits(got.var, np.var(a, axis=0, ddof=1))
                and np.array_equal(got.min, a.min(axis=0)) and np.array_equal(got.max, a.max(axis=0))):
            raise SystemExit(f"{cfg}: statistics differ from numpy")
        del a, got
        call()
        t_call = timed(call) / args.calls
        nbytes = 8 * (B + 4) * (n + 2) ** 2

        def loop():  # through the C ABI: the results stay in the pinned buffers
            for _ in range(args.loops):
                if lib.csim_ensemble_stats_begin(e._h, 1) or lib.csim_ensemble_run(e._h, RUN) or \
                        lib.csim_ensemble_stats_wait(e._h, None, None, None, None):
                    raise SystemExit(lib.csim_last_error().decode())

        def loop_py():  # Ensemble.stats_wait() copies the four fields into numpy arrays
            for _ in range(args.loops):
                e.stats_begin(1)
                e.run(RUN)
                e.stats_wait()

        def runs():
            for _ in range(args.loops):
                e.run(RUN)
            e.sync()
        loop()
        runs()
        loop_py()
        t_loop, t_run, t_py = timed(loop) / args.loops, timed(runs) / args.loops, timed(loop_py) / args.loops
        rec = dict(config=cfg, members=B, n=n, compulsory_bytes=nbytes, calls=args.calls,
                   stats_call_us=t_call * 1e6, stats_gbps=nbytes / t_call / 1e9,
                   run20_us=t_run * 1e6, loop_us=t_loop * 1e6, loop_ratio=t_loop / t_run,
                   loop_over_run_plus_stats=t_loop / (t_run + t_call), loop_python_us=t_py * 1e6,
                   step_us=t_run / RUN * 1e6, stats_over_step=t_call / (t_run / RUN))
        e.close()
        line = json.dumps(rec)
        print(line, flush=True)
        if args.out:
            with open(args.out, "a") as f:
                f.write(line + "\n")


if __name__ == "__main__":
    main()
