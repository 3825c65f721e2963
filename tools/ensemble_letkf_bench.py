#!/usr/bin/env python3
"""tools/ensemble_letkf_bench.py — cost of the LETKF (csim_ensemble_assimilate_letkf) at node spacings 4, 8 and 16 beside
the serial filter and the local analysis on the same networks, one JSON line per network.  The networks and the
forecast members (member 0 is the truth) are those of tools/ensemble_local_bench.py; the method is that of the other
ensemble tools: the host clock around call + sync with the members uploaded afresh outside the timed part, --calls calls
per region, five regions, the median and the spread (max - min) / median.

Per spacing s:
  letkf_s{s}_us          csim_ensemble_assimilate_letkf, then a sync;
  letkf_s{s}_enqueue_us  the host time of the call alone, the sync outside the timed part;
  letkf_s{s}_nodes, _bytes   csim_letkf_plan; "unsupported" in letkf_s{s}_status where the plan exceeds the limits.
serial_us and local_us are csim_ensemble_assimilate_network and csim_ensemble_assimilate_local (local_status
"unsupported" beyond its limits).  With --accuracy (the second network by default) the line also holds, per spacing,
rms_vs_local_s{s}: the RMS difference of the analysis mean from that of the local analysis, which is the LETKF with a
node on every cell in exact arithmetic (one node per cell on 256^2 is beyond CSIM_LETKF_MAX_NODES), relative to the RMS
increment of the local analysis: the accuracy that the spacing costs.
With --only S the program makes --calls analyses at spacing S on the first network and exits, for a kernel trace.

  python tools/ensemble_letkf_bench.py [--config 64x512:lattice16 ...] [--spacing 4,8,16] [--out FILE]
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

R = 0.5
REGIONS = 5
# 64 x 512^2 with 1024 observations; 64 x 256^2 with 1024 random ones; 64 x 256^2 with one on every fourth cell;
# 256 x 256^2 with 1024 random ones, which is outside the local analysis's limits
DEFAULT = ["64x512:lattice16", "64x256:random1024", "64x256:lattice4", "256x256:random1024"]


def observations(kind, n, rng):
    if kind.startswith("lattice"):
        s = int(kind[len("lattice"):])
        g = np.arange(max(s // 2, 1), n + 1, s)
        I, J = np.meshgrid(g, g)
        i, j = I.ravel(), J.ravel()
    else:
        k = int(kind[len("random"):])
        i, j = rng.integers(1, n + 1, k), rng.integers(1, n + 1, k)
    return i.astype(np.int32), j.astype(np.int32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", action="append", default=[], help="BxN:OBS, OBS = latticeS or randomK")
    ap.add_argument("--spacing", default="4,8,16")
    ap.add_argument("--loc", type=float, default=8.0)
    ap.add_argument("--calls", type=int, default=3, help="analyses per timed region")
    ap.add_argument("--accuracy", default="64x256:random1024", help="the network whose line gets rms_vs_local")
    ap.add_argument("--only", type=int, help="only --calls analyses at this spacing on the first network")
    ap.add_argument("--out", help="append the JSON lines to this file too")
    args = ap.parse_args()
    pkg = load_package()
    pkg.set_device(0)
    spacings = [int(v) for v in args.spacing.split(",") if v]
    for cfg in args.config or DEFAULT:
        size, kind = cfg.split(":")
        B, n = (int(v) for v in size.split("x"))
        rng = np.random.default_rng(B * 7 + n)
        i, j = observations(kind, n, rng)
        nobs = len(i)
        y = rng.standard_normal(nobs)
        X = rng.standard_normal((B, n + 2, n + 2))
        e = pkg.Ensemble(B, n, n, 1.0, 1.0, [0, 0, 0, 0])
        e.upload_all(X)
        net = e.obs_network(i, j, R, args.loc)
        net.set_values(y)
        if args.only:
            for _ in range(args.calls):
                e.assimilate_letkf(net, truth_member=0, spacing=args.only)
                e.sync()
            e.close()
            return
        rec = dict(config=cfg, members=B, forecast=B - 1, n=n, nobs=nobs, loc=args.loc, calls=args.calls,
                   regions=REGIONS, max_local=net.local_info())

        def measure(call, enqueue_only=False):
            """(median, spread) in microseconds per call"""
            def region():
                total = 0.0
                for _ in range(args.calls):
                    e.upload_all(X)
                    e.sync()
                    t0 = time.perf_counter()
                    call()
                    if enqueue_only:
                        total += time.perf_counter() - t0
                        e.sync()
                    else:
                        e.sync()
                        total += time.perf_counter() - t0
                return total / args.calls * 1e6
            region()
            out = [region() for _ in range(REGIONS)]
            med = statistics.median(out)
            return med, (max(out) - min(out)) / med

        def changed(what):
            A = e.download_all()
            if not np.isfinite(A).all() or np.array_equal(A[1:], X[1:]) or not np.array_equal(A[0], X[0]):
                raise SystemExit(f"{cfg}: {what} left members that are not finite, or unchanged")
            return A[1:, 1:-1, 1:-1].mean(axis=0)

        mean_b = X[1:, 1:-1, 1:-1].mean(axis=0)
        mean_local = None
        try:
            e.assimilate_local(net, truth_member=0)
            mean_local = changed("the local analysis")
            rec["local_us"], rec["local_spread"] = measure(lambda: e.assimilate_local(net, truth_member=0))
            rec["local_status"] = "ok"
        except pkg.CsimError as err:
            if err.code != 5:
                raise
            rec["local_status"] = "unsupported"
        rec["serial_us"], rec["serial_spread"] = measure(lambda: e.assimilate_network(net, truth_member=0))
        for s in spacings:
            plan = pkg.letkf_plan(B - 1, n, n, s)
            rec[f"letkf_s{s}_nodes"], rec[f"letkf_s{s}_bytes"] = plan.nodes, plan.bytes
            call = lambda: e.assimilate_letkf(net, truth_member=0, spacing=s)  # noqa: E731
            try:
                e.upload_all(X)
                call()
                mean_s = changed(f"the LETKF at spacing {s}")
            except pkg.CsimError as err:
                if err.code != 5:
                    raise
                rec[f"letkf_s{s}_status"] = "unsupported"
                continue
            info = e.letkf_info()
            rec[f"letkf_s{s}_status"] = "ok"
            rec[f"letkf_s{s}_idle_nodes"] = int((info.status == pkg.LETKF_IDLE).sum())
            rec[f"letkf_s{s}_max_count"], rec[f"letkf_s{s}_max_sweeps"] = int(info.count.max()), int(info.sweeps.max())
            if cfg == args.accuracy and mean_local is not None:
                rec[f"rms_vs_local_s{s}"] = float(np.sqrt(np.mean((mean_s - mean_local) ** 2))
                                                  / np.sqrt(np.mean((mean_local - mean_b) ** 2)))
            rec[f"letkf_s{s}_us"], rec[f"letkf_s{s}_spread"] = measure(call)
            rec[f"letkf_s{s}_enqueue_us"], rec[f"letkf_s{s}_enqueue_spread"] = measure(call, enqueue_only=True)
            rec[f"letkf_s{s}_over_serial"] = rec[f"letkf_s{s}_us"] / rec["serial_us"]
        e.close()
        line = json.dumps(rec)
        print(line, flush=True)
        if args.out:
            with open(args.out, "a") as f:
                f.write(line + "\n")


if __name__ == "__main__":
    main()
