#!/usr/bin/env python3
"""tools/ensemble_obsop_bench.py — what linear observations (csim_obs_network_create_linear) cost against point
observations on the same anchors, one JSON line per configuration.

For B members of n x n (Dirichlet on all sides, member 0 the truth, so M = B - 1) and a lattice of anchors, four
networks: the point network, and linear networks of one tap (0, 0, 1.0), four taps (bilinear to the cell centre plus
(0.5, 0.5)) and 25 taps (the 5 x 5 box mean).  The one-tap network is first checked bit for bit against the point
network on a copy of the state (a random field has no zeros).  Then, per network, the mean over `--calls` calls of
assimilate_network plus the stream sync, each call starting on an idle stream, median of `--regions` regions after one
warm-up region:
  point_sync_us, tap1_sync_us, tap4_sync_us, tap25_sync_us     the analysis (prior and update launches of every batch)
  *_record_sync_us                                             with record = 1 (the two diagnostic launches, the log)
  *_observe_sync_us                                            observe with noise
The update kernel is the same for all four, so the differences are the linear prior's (and, with a record, the linear
diagnostics').  Kernel times come from a rocprofv3 --kernel-trace --stats run of `--only-kernels`.

  python tools/ensemble_obsop_bench.py --config 65x512:lattice16 --config 1025x128:lattice16 [--out F]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", action="append", default=[], help="BxN:latticeS")
    ap.add_argument("--loc", type=float, default=8.0)
    ap.add_argument("--calls", type=int, default=20, help="calls per timed region")
    ap.add_argument("--regions", type=int, default=5)
    ap.add_argument("--only-kernels", action="store_true", help="only --calls recorded analyses per network (profiler)")
    ap.add_argument("--out", help="append the JSON lines to this file too")
    args = ap.parse_args()
    pkg = load_package()
    pkg.set_device(0)
    for cfg in args.config or ["65x512:lattice16", "1025x128:lattice16"]:
        size, kind = cfg.split(":")
        B, n = (int(v) for v in size.split("x"))
        s = int(kind[len("lattice"):])
        g = np.arange(s // 2, n, s)                      # anchors at least 2 cells from every side for s >= 6
        I, J = np.meshgrid(g, g)
        i, j = I.ravel().astype(np.int32), J.ravel().astype(np.int32)
        nobs = len(i)
        rng = np.random.default_rng(B * 7 + n)
        X = rng.standard_normal((B, n + 2, n + 2))
        y = rng.standard_normal(nobs)
        one = (np.arange(nobs + 1, dtype=np.int32), np.zeros(nobs, dtype=np.int32), np.zeros(nobs, dtype=np.int32),
               np.ones(nobs))
        taps = {"point": None, "tap1": one, "tap4": pkg.bilinear_taps(n, n, i + 0.5, j + 0.5)[2],
                "tap25": pkg.box_taps(n, n, i, j, 2, 2)[2]}
        assert len(taps["tap4"].w) == 4 * nobs and len(taps["tap25"].w) == 25 * nobs
        rec = dict(config=cfg, members=B, forecast=B - 1, n=n, nobs=nobs, loc=args.loc, calls=args.calls,
                   regions=args.regions)

        if not args.only_kernels:
            got = []
            for name in ("point", "tap1"):
                e = pkg.Ensemble(B, n, n, 1.0, 1.0, [0, 0, 0, 0])
                e.upload_all(X)
                net = e.obs_network(i, j, R, args.loc, taps=taps[name])
                net.set_values(y)
                e.assimilate_network(net, truth_member=0)
                got.append(e.download_all())
                e.close()
            if not np.array_equal(got[0].view(np.int64), got[1].view(np.int64)):
                raise SystemExit(f"{cfg}: the one-tap network differs from the point network")

        e = pkg.Ensemble(B, n, n, 1.0, 1.0, [0, 0, 0, 0])
        e.upload_all(X)
        nets = {k: e.obs_network(i, j, R, args.loc, log_cycles=args.calls * (args.regions + 1), taps=t)
                for k, t in taps.items()}
        rec["nlevels"] = nets["point"].info.nlevels
        for net in nets.values():
            net.set_values(y)

        if args.only_kernels:
            for net in nets.values():
                for _ in range(args.calls):
                    e.assimilate_network(net, truth_member=0, record=True)
                    e.sync()
                net.log_reset()
            e.close()
            continue

        def region(fn):
            total = 0.0
            for _ in range(args.calls):
                t0 = time.perf_counter()
                fn()
                e.sync()
                total += time.perf_counter() - t0
            return total / args.calls * 1e6

        # interleaved: every region of every network before the next round, so that drift shows in all alike
        forms = {"sync": lambda net: e.assimilate_network(net, truth_member=0),
                 "record_sync": lambda net: e.assimilate_network(net, truth_member=0, record=True),
                 "observe_sync": lambda net: net.observe(0, 5, 1)}
        for form, call in forms.items():
            samples = {k: [] for k in nets}
            for rnd in range(args.regions + 1):
                for k, net in nets.items():
                    v = region(lambda: call(net))
                    if rnd:
                        samples[k].append(v)
            for k in nets:
                rec[f"{k}_{form}_us"] = statistics.median(samples[k])
                rec[f"{k}_{form}_samples_us"] = [round(v, 2) for v in samples[k]]
            for net in nets.values():
                net.log_reset()
                net.set_values(y)
        for k in ("tap1", "tap4", "tap25"):
            rec[f"{k}_over_point"] = rec[f"{k}_sync_us"] / rec["point_sync_us"]
        e.close()
        line = json.dumps(rec)
        print(line, flush=True)
        if args.out:
            with open(args.out, "a") as f:
                f.write(line + "\n")


if __name__ == "__main__":
    main()
