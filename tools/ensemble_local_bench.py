#!/usr/bin/env python3
"""tools/ensemble_local_bench.py — the local analysis (csim_ensemble_assimilate_local) beside the serial one
(csim_ensemble_assimilate_network) on the same networks, one JSON line per configuration.

For B members of n x n (Dirichlet on all sides, member 0 the truth, so M = B - 1) and one network, in one process and
one build, the mean over `--calls` analyses that each start on an idle stream and end with a stream sync, median of three
regions after a warm-up region.  Every analysis starts from the same uploaded state (the upload is outside the timed
part).  The serial path is not touched by the local analysis, so serial_us is what the library gave before it.
  local_us     assimilate_local: the observation priors and the cell pass, two launches
  serial_us    assimilate_network: two launches per batch of a level
  max_local    the network's bound (ObsNetwork.local_info()); nlevels: the serial plan's levels
  status       "ok", or "unsupported" where the network is beyond the limits of the local analysis (CSIM_LOCAL_MAX_OBS
               windows over a cell, CSIM_LOCAL_MAX_DOUBLES private priors per cell): then only serial_us is measured
The two analyses are different estimators (the local one is order-independent), so their members are not compared; the
tool checks that both leave finite members and that the local one changed them.

  python tools/ensemble_local_bench.py [--config 64x512:lattice16 ...] [--loc 8] [--calls 20] [--out F]

The kernel split comes from a run of its own:  rocprofv3 --kernel-trace --stats -- python tools/ensemble_local_bench.py ...
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
# the three networks of DESIGN 7f's table, the random one again with an ensemble that fits the per-cell bound, and a
# dense one: an observation on every fourth cell
DEFAULT = ["64x512:lattice16", "64x1024:lattice16", "256x256:random1024", "64x256:random1024", "64x256:lattice4"]


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
    ap.add_argument("--loc", type=float, default=8.0)
    ap.add_argument("--calls", type=int, default=20, help="analyses per timed region")
    ap.add_argument("--out", help="append the JSON lines to this file too")
    args = ap.parse_args()
    pkg = load_package()
    pkg.set_device(0)
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
        rec = dict(config=cfg, members=B, forecast=B - 1, n=n, nobs=nobs, loc=args.loc, calls=args.calls,
                   nlevels=net.info.nlevels, max_local=net.local_info(), status="ok")

        def measure(call):
            def region():
                total = 0.0
                for _ in range(args.calls):
                    e.upload_all(X)
                    e.sync()
                    t0 = time.perf_counter()
                    call()
                    e.sync()
                    total += time.perf_counter() - t0
                return total
            region()
            return statistics.median(region() for _ in range(3)) / args.calls * 1e6

        try:
            e.assimilate_local(net, truth_member=0)
            A = e.download_all()
            if not np.isfinite(A).all() or np.array_equal(A[1:], X[1:]) or not np.array_equal(A[0], X[0]):
                raise SystemExit(f"{cfg}: the local analysis left members that are not finite, or unchanged")
            rec["local_us"] = measure(lambda: e.assimilate_local(net, truth_member=0))
        except pkg.CsimError as err:
            if err.code != 5:
                raise
            rec["status"] = "unsupported"
        rec["serial_us"] = measure(lambda: e.assimilate_network(net, truth_member=0))
        if not np.isfinite(e.download_all()).all():
            raise SystemExit(f"{cfg}: the serial analysis left members that are not finite")
        if "local_us" in rec:
            rec["local_over_serial"] = rec["local_us"] / rec["serial_us"]
        e.close()
        line = json.dumps(rec)
        print(line, flush=True)
        if args.out:
            with open(args.out, "a") as f:
                f.write(line + "\n")


if __name__ == "__main__":
    main()
