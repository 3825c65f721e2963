#!/usr/bin/env python3
"""tools/ensemble_obsnet_bench.py — what a device-resident observation network (csim_obs_network_*) saves, one JSON line
per configuration.

For B members of n x n (Dirichlet on all sides, the same advection physics for every member, member 0 the truth, so
M = B - 1), after the analysed members of assimilate_network have been checked bit for bit against
csim_ensemble_assimilate on a copy of the state, in one process, the mean over `--calls` calls, median of three regions:
  host_call_us / net_call_us   (a) host time until the call returns: csim_ensemble_assimilate without diagnostics (the
                               unchanged entry point) and assimilate_network without a record; the stream is idle when
                               each call starts
  host_sync_us / net_sync_us   (b) the call plus the stream sync
  net_record_sync_us           (b) with record = 1 (two diagnostic launches and the two of the log more)
  osse_host_us / osse_net_us   (c) per cycle of a 20-cycle OSSE, run(20) -> observe -> prior_capture -> analysis -> relax
                               -> perturb: the host loop (download the truth, numpy noise, csim_ensemble_assimilate) and
                               the enqueued form (observe and assimilate_network(record), one log() at the end)
Kernel times come from a rocprofv3 --kernel-trace --stats run of `--only-kernels` (only `--calls` calls of observe and of
the recorded analysis, no check, no host loop).

  python tools/ensemble_obsnet_bench.py --config 64x512:lattice16 --config 64x1024:lattice16 \
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
from __graft_entry__ import load_package  # noqa: E402

D, VX, VY = 0.05, 0.5, 0.25
RUN = 20
R = 0.5
CYCLES = 20


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
    return i.astype(np.int32), j.astype(np.int32)


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.int64), b.view(np.int64))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", action="append", default=[], help="BxN:OBS, OBS = latticeS or randomK")
    ap.add_argument("--loc", type=float, default=8.0)
    ap.add_argument("--calls", type=int, default=20, help="calls per timed region")
    ap.add_argument("--only-kernels", action="store_true", help="only --calls calls of each kernel (profiler)")
    ap.add_argument("--out", help="append the JSON lines to this file too")
    args = ap.parse_args()
    pkg = load_package()
    pkg.set_device(0)
    dt = min(0.1, pkg.safe_dt(1.0, 1.0, VX, VY, D))
    for cfg in args.config or ["64x512:lattice16", "64x1024:lattice16", "256x256:random1024"]:
        size, kind = cfg.split(":")
        B, n = (int(v) for v in size.split("x"))
        rng = np.random.default_rng(B * 7 + n)
        i, j = observations(kind, n, rng)
        nobs = len(i)
        y = rng.standard_normal(nobs)
        X = rng.standard_normal((B, n + 2, n + 2))
        e = pkg.Ensemble(B, n, n, 1.0, 1.0, [0, 0, 0, 0])
        e.upload_all(X)
        e.set_physics(D, dt, VX, VY)
        net = e.obs_network(i, j, R, args.loc, log_cycles=max(args.calls * 4, CYCLES))
        rec = dict(config=cfg, members=B, n=n, nobs=nobs, nlevels=net.info.nlevels, loc=args.loc, calls=args.calls)

        if args.only_kernels:
            for _ in range(args.calls):
                net.observe(0, 1, 0)
                e.assimilate_network(net, truth_member=0, record=True)
                e.sync()
                net.log_reset()
            e.close()
            continue

        other = pkg.Ensemble(B, n, n, 1.0, 1.0, [0, 0, 0, 0])
        other.upload_all(X)
        net.set_values(y)
        e.assimilate_network(net, truth_member=0)
        other.assimilate(i, j, y, R, args.loc, truth_member=0, diagnostics=False)
        if not same_bits(e.download_all(), other.download_all()):
            raise SystemExit(f"{cfg}: assimilate_network differs from csim_ensemble_assimilate")
        other.close()

        def calls(fn, with_sync):
            """mean time of fn (and the sync, if asked for) over --calls calls that each start on an idle stream"""
            def region():
                total = 0.0
                for _ in range(args.calls):
                    t0 = time.perf_counter()
                    fn()
                    if with_sync:
                        e.sync()
                    total += time.perf_counter() - t0
                    e.sync()
                return total
            region()
            return timed(region) / args.calls * 1e6

        host = lambda: e.assimilate(i, j, y, R, args.loc, truth_member=0, diagnostics=False)
        plain = lambda: e.assimilate_network(net, truth_member=0)

        def recorded():
            e.assimilate_network(net, truth_member=0, record=True)

        rec["host_call_us"], rec["net_call_us"] = calls(host, False), calls(plain, False)
        rec["host_sync_us"], rec["net_sync_us"] = calls(host, True), calls(plain, True)
        net.log_reset()
        rec["net_record_sync_us"] = calls(recorded, True)
        net.log_reset()

        noise = np.random.default_rng(1)

        def osse_host():
            for c in range(CYCLES):
                e.run(RUN)
                truth = e.download(0)
                yy = truth[j, i] + np.sqrt(R) * noise.standard_normal(nobs)
                e.prior_capture("spread", truth_member=0)
                e.assimilate(i, j, yy, R, args.loc, truth_member=0, diagnostics=False)
                e.relax(0.5, truth_member=0)
                e.perturb(0.01, 3.0, 5, c, truth_member=0)
            e.sync()

        def osse_net():
            net.log_reset()
            for c in range(CYCLES):
                e.run(RUN)
                net.observe(0, 5, c)
                e.prior_capture("spread", truth_member=0)
                e.assimilate_network(net, truth_member=0, record=True)
                e.relax(0.5, truth_member=0)
                e.perturb(0.01, 3.0, 5, c, truth_member=0)
            assert len(net.log()) == CYCLES

        e.upload_all(X)
        osse_host()
        osse_net()
        rec["osse_host_us"] = timed(osse_host) / CYCLES * 1e6
        rec["osse_net_us"] = timed(osse_net) / CYCLES * 1e6
        rec["call_saved_us"] = rec["host_call_us"] - rec["net_call_us"]
        rec["sync_saved_us"] = rec["host_sync_us"] - rec["net_sync_us"]
        rec["osse_saved_us"] = rec["osse_host_us"] - rec["osse_net_us"]
        e.close()
        line = json.dumps(rec)
        print(line, flush=True)
        if args.out:
            with open(args.out, "a") as f:
                f.write(line + "\n")


if __name__ == "__main__":
    main()
