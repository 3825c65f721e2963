#!/usr/bin/env python3
"""tools/ensemble_assim_bench.py — cost of the ensemble analysis (csim_ensemble_assimilate), one JSON line per
configuration.

For B members of n x n (Dirichlet on all sides, the same advection physics for every member, M = B forecast members)
and observations on a lattice or at random cells, Gaspari-Cohn length `--loc` cells (unit spacing), error variance 0.5:
  nlevels         the plan's level count (first fit);
  call_us         one csim_ensemble_assimilate without diagnostics followed by a stream sync (the observations' copy,
                  every launch, the kernels), the mean over `--calls` calls, median of three regions;
  diag_call_us    the same with all four diagnostics (synchronous, plus the posterior launch and the copies back);
  eff_gbps        the effective bytes 16 M x (window cells with rho > 0, summed over the observations) over call_us
                  (each touched member value read once and written once);
  loop_ratio      `--loops` x (assimilate without diagnostics; run(20)) against `--loops` x run(20), then one sync;
  host_s          the host path of the same analysis: download_all, the numpy restatement of
                  tests/test_gpu_ensemble_assim.py (serial, vectorised over each window), upload_all; its result is
                  also the check that the GPU analysis of the same fields is bit for bit the restatement's.
Kernel times come from a rocprofv3 --kernel-trace --stats run of `--only-assim` (only `--calls` analyses, no host
path).

  python tools/ensemble_assim_bench.py --config 64x512:lattice16 --config 64x1024:lattice16 \
      --config 256x256:random1024 [--out F]
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
from test_gpu_ensemble_assim import restate, same_bits  # noqa: E402

D, VX, VY = 0.05, 0.5, 0.25
RUN = 20
R = 0.5


def timed(fn, regions=3):
    out = []
    for _ in range(regions):
        t0 = time.perf_counter()
        fn()
        out.append(time.perf_counter() - t0)
    return statistics.median(out)


def observations(kind, n, rng):
    if kind.startswith("lattice"):
        s = int(kind[len("lattice"):])
        g = np.arange(s // 2, n + 1, s)
        I, J = np.meshgrid(g, g)
        i, j = I.ravel(), J.ravel()
    else:
        k = int(kind[len("random"):])
        i, j = rng.integers(1, n + 1, k), rng.integers(1, n + 1, k)
    return i.astype(np.int32), j.astype(np.int32), rng.standard_normal(len(i))


def touched_cells(pkg, n, loc, i, j):
    rho = pkg.ensemble_gc_table(1.0, 1.0, loc, n, n)
    ly, lx = (rho.shape[0] - 1) // 2, (rho.shape[1] - 1) // 2
    total = 0
    for io, jo in zip(i, j):
        i0, i1, j0, j1 = max(1, io - lx), min(n, io + lx), max(1, jo - ly), min(n, jo + ly)
        total += int((rho[j0 - jo + ly:j1 - jo + ly + 1, i0 - io + lx:i1 - io + lx + 1] > 0).sum())
    return total


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", action="append", default=[], help="BxN:OBS, OBS = latticeS or randomK")
    ap.add_argument("--loc", type=float, default=8.0)
    ap.add_argument("--calls", type=int, default=20, help="analyses per timed region")
    ap.add_argument("--loops", type=int, default=10, help="assimilate / run iterations per timed region")
    ap.add_argument("--only-assim", action="store_true", help="only --calls analyses per configuration (profiler)")
    ap.add_argument("--no-host", action="store_true", help="skip the host path and its bit-for-bit check")
    ap.add_argument("--out", help="append the JSON lines to this file too")
    args = ap.parse_args()
    pkg = load_package()
    pkg.set_device(0)
    C = pkg.C
    lib = pkg.lib()
    dt = min(0.1, pkg.safe_dt(1.0, 1.0, VX, VY, D))
    ip, dp = C.POINTER(C.c_int), C.POINTER(C.c_double)
    for cfg in args.config or ["64x512:lattice16", "64x1024:lattice16", "256x256:random1024"]:
        size, kind = cfg.split(":")
        B, n = (int(v) for v in size.split("x"))
        rng = np.random.default_rng(B * 7 + n)
        i, j, y = observations(kind, n, rng)
        r = np.full(len(i), R)
        e = pkg.Ensemble(B, n, n, 1.0, 1.0, [0, 0, 0, 0])
        X = rng.standard_normal((B, n + 2, n + 2))
        e.upload_all(X)
        e.set_physics(D, dt, VX, VY)
        pi, pj, py, pr = i.ctypes.data_as(ip), j.ctypes.data_as(ip), y.ctypes.data_as(dp), r.ctypes.data_as(dp)
        nl = C.c_int()

        def enqueue():
            if lib.csim_ensemble_assimilate(e._h, len(i), pi, pj, py, pr, args.loc, 1.0, -1, 0, None, None, None, None,
                                            C.byref(nl)):
                raise SystemExit(lib.csim_last_error().decode())

        def call():
            for _ in range(args.calls):
                enqueue()
                e.sync()
        if args.only_assim:
            call()
            e.close()
            continue
        rec = dict(config=cfg, members=B, n=n, nobs=len(i), loc=args.loc)
        if not args.no_host:
            t0 = time.perf_counter()
            A = e.download_all()
            W = restate(pkg, A, 1.0, 1.0, i, j, y, r, args.loc, 1.0, -1, False)[0]
            e.upload_all(W)
            rec["host_s"] = time.perf_counter() - t0
            e.upload_all(X)
            e.assimilate(i, j, y, r, args.loc, diagnostics=False)
            if not same_bits(e.download_all(), W):
                raise SystemExit(f"{cfg}: the analysis differs from the numpy restatement")
            del A, W
        call()
        t_call = timed(call) / args.calls
        pm, pv, qm, qv = (np.empty(len(i)) for _ in range(4))

        def diag():
            for _ in range(args.calls):
                if lib.csim_ensemble_assimilate(e._h, len(i), pi, pj, py, pr, args.loc, 1.0, -1, 0,
                                                *[a.ctypes.data_as(dp) for a in (pm, pv, qm, qv)], C.byref(nl)):
                    raise SystemExit(lib.csim_last_error().decode())
        diag()
        t_diag = timed(diag) / args.calls

        def loop():
            for _ in range(args.loops):
                enqueue()
                e.run(RUN)
            e.sync()

        def runs():
            for _ in range(args.loops):
                e.run(RUN)
            e.sync()
        loop()
        runs()
        t_loop, t_run = timed(loop) / args.loops, timed(runs) / args.loops
        cells = touched_cells(pkg, n, args.loc, i, j)
        nbytes = 16 * B * cells
        rec.update(nlevels=nl.value, touched_cells=cells, eff_bytes=nbytes, calls=args.calls, call_us=t_call * 1e6,
                   diag_call_us=t_diag * 1e6, eff_gbps=nbytes / t_call / 1e9, run20_us=t_run * 1e6,
                   loop_us=t_loop * 1e6, loop_ratio=t_loop / t_run, loop_minus_run_us=(t_loop - t_run) * 1e6)
        if "host_s" in rec:
            rec["host_over_call"] = rec["host_s"] / t_call
        e.close()
        line = json.dumps(rec)
        print(line, flush=True)
        if args.out:
            with open(args.out, "a") as f:
                f.write(line + "\n")


if __name__ == "__main__":
    main()
