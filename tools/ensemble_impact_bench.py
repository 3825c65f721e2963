#!/usr/bin/env python3
"""tools/ensemble_impact_bench.py — what the per-observation forecast impact costs (csim_obs_network_impact_capture,
csim_ensemble_obs_impact), one JSON line per configuration, on the network shapes of tools/ensemble_assim_bench.py.

For B members of n x n (Dirichlet on all sides, member 0 the truth, so M = B - 1) and one network, in one process: the
mean over `--calls` calls that each start on an idle stream and end with a stream sync, over `--regions` regions after a
warm-up region; median, and the least and the largest region as the spread.
  assim_us     assimilate_network without a record, each from the same uploaded state (the upload is outside the timed
               part): the yardstick.  It reads the same windows and also writes them.  Its kernels are those of the
               revision before the impact existed
  capture_us   impact_capture after a recorded analysis: nobs x M values read, as many written
  impact_us    obs_impact on the analysed state: the weight's copy to the device, the kernel, the copy of nobs values
               back and the summary; the call is synchronous
  impact_ratio = impact_us / assim_us, capture_ratio = capture_us / assim_us
The result is checked against a second call (the same bits) before anything is timed.

  python tools/ensemble_impact_bench.py --config 64x512:lattice16 --config 256x256:random1024 [--out F]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", action="append", default=[], help="BxN:OBS, OBS = latticeS or randomK")
    ap.add_argument("--loc", type=float, default=8.0)
    ap.add_argument("--calls", type=int, default=10, help="calls per timed region")
    ap.add_argument("--regions", type=int, default=5, help="timed regions per number, after one warm-up region")
    ap.add_argument("--out", help="append the JSON lines to this file too")
    args = ap.parse_args()
    pkg = load_package()
    pkg.set_device(0)
    for cfg in args.config or ["64x512:lattice16", "64x1024:lattice16", "256x256:random1024"]:
        size, kind = cfg.split(":")
        B, n = (int(v) for v in size.split("x"))
        rng = np.random.default_rng(B * 7 + n)
        i, j = observations(kind, n, rng)
        nobs = len(i)
        y = rng.standard_normal(nobs)
        X = rng.standard_normal((B, n + 2, n + 2))
        w = rng.standard_normal((n + 2, n + 2))
        e = pkg.Ensemble(B, n, n, 1.0, 1.0, [0, 0, 0, 0])
        net = e.obs_network(i, j, R, args.loc, log_cycles=1)
        net.set_values(y)
        info = net.info
        rec = dict(config=cfg, members=B, n=n, nobs=nobs, nlevels=info.nlevels, loc=args.loc,
                   window=(2 * info.lx + 1) * (2 * info.ly + 1), calls=args.calls, regions=args.regions)
        e.upload_all(X)
        e.assimilate_network(net, truth_member=0, record=True)
        net.impact_capture(truth_member=0)
        first, second = e.obs_impact(net, w), e.obs_impact(net, w)
        if first.impact.tobytes() != second.impact.tobytes() or first.summary != second.summary:
            raise SystemExit(f"{cfg}: two evaluations of one capture differ")
        if not np.isfinite(first.impact).all() or first.summary.used != nobs:
            raise SystemExit(f"{cfg}: the impact is not finite")
        rec["beneficial"], rec["total"] = first.summary.beneficial, first.summary.total

        def measure(call, before=lambda: None):
            def region():
                total = 0.0
                for _ in range(args.calls):
                    before()
                    e.sync()
                    t0 = time.perf_counter()
                    call()
                    e.sync()
                    total += time.perf_counter() - t0
                return total / args.calls * 1e6
            region()
            t = sorted(region() for _ in range(args.regions))
            return statistics.median(t), t[0], t[-1]

        # capture and impact first: they need the recorded analysis to be the network's last
        for key, call, before in (("capture", lambda: net.impact_capture(truth_member=0), lambda: None),
                                  ("impact", lambda: e.obs_impact(net, w), lambda: None),
                                  ("assim", lambda: e.assimilate_network(net, truth_member=0), lambda: e.upload_all(X))):
            rec[key + "_us"], rec[key + "_min_us"], rec[key + "_max_us"] = measure(call, before)
        rec["impact_ratio"] = rec["impact_us"] / rec["assim_us"]
        rec["capture_ratio"] = rec["capture_us"] / rec["assim_us"]
        e.close()
        line = json.dumps(rec)
        print(line, flush=True)
        if args.out:
            with open(args.out, "a") as f:
                f.write(line + "\n")


if __name__ == "__main__":
    main()
