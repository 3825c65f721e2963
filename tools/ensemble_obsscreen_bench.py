#!/usr/bin/env python3
"""tools/ensemble_obsscreen_bench.py — what screening an observation network costs (csim_obs_network_set_active,
csim_ensemble_assimilate_screened), one JSON line per configuration.

For B members of n x n (Dirichlet on all sides, member 0 the truth, so M = B - 1) and one network, in one process, the
mean over `--calls` analyses that each start on an idle stream and end with a stream sync, median of three regions.
Every analysis starts from the same uploaded state (the upload is outside the timed part), so all forms do the same
arithmetic on the same numbers:
  plain_us            assimilate_network without screening: the launches of before
  screened_us         screen = 1e6, a tolerance that rejects nothing (checked: every status 0, the members bit for bit
                      those of the plain analysis): one (hb, vb) pass over nobs x M values and the nobs-lane
                      k_obs_screen more, and a null test per block in the analysis kernels
  plain_record_us / screened_record_us   the same with record = 1 (the (hb, vb) pass is the record's own there)
  inactive_us         screen = 0 with a share `--inactive` of the observations masked out: their blocks are launched
                      and leave at once
  screen_ratio = screened_us / plain_us, record_ratio, inactive_ratio = inactive_us / plain_us

  python tools/ensemble_obsscreen_bench.py --config 64x512:lattice16 --config 256x256:random1024 [--inactive 0.3] [--out F]
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
NOTHING = 1e6   # a tolerance that rejects nothing


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
    ap.add_argument("--calls", type=int, default=10, help="analyses per timed region")
    ap.add_argument("--inactive", type=float, default=0.3, help="share of the observations masked out in inactive_us")
    ap.add_argument("--out", help="append the JSON lines to this file too")
    args = ap.parse_args()
    pkg = load_package()
    pkg.set_device(0)
    for cfg in args.config or ["64x512:lattice16", "256x256:random1024"]:
        size, kind = cfg.split(":")
        B, n = (int(v) for v in size.split("x"))
        rng = np.random.default_rng(B * 7 + n)
        i, j = observations(kind, n, rng)
        nobs = len(i)
        y = rng.standard_normal(nobs)
        X = rng.standard_normal((B, n + 2, n + 2))
        e = pkg.Ensemble(B, n, n, 1.0, 1.0, [0, 0, 0, 0])
        net = e.obs_network(i, j, R, args.loc, log_cycles=args.calls)
        net.set_values(y)
        mask = (rng.uniform(size=nobs) >= args.inactive).astype(np.uint8)
        rec = dict(config=cfg, members=B, n=n, nobs=nobs, nlevels=net.info.nlevels, loc=args.loc, calls=args.calls,
                   inactive=int(nobs - mask.sum()))

        def analysed(**kw):
            e.upload_all(X)
            e.assimilate_network(net, truth_member=0, **kw)
            return e.download_all()

        net.set_active(None)
        want = analysed()
        got = analysed(screen=NOTHING)
        if net.status().any() or not same_bits(got, want):
            raise SystemExit(f"{cfg}: a screened analysis that rejects nothing differs from the plain one")

        def measure(**kw):
            def region():
                total = 0.0
                net.log_reset()
                for _ in range(args.calls):
                    e.upload_all(X)
                    e.sync()
                    t0 = time.perf_counter()
                    e.assimilate_network(net, truth_member=0, **kw)
                    e.sync()
                    total += time.perf_counter() - t0
                return total
            region()
            return statistics.median(region() for _ in range(3)) / args.calls * 1e6

        rec["plain_us"] = measure()
        rec["screened_us"] = measure(screen=NOTHING)
        rec["plain_record_us"] = measure(record=True)
        rec["screened_record_us"] = measure(record=True, screen=NOTHING)
        net.set_active(mask)
        rec["inactive_us"] = measure()
        rec["screen_ratio"] = rec["screened_us"] / rec["plain_us"]
        rec["record_ratio"] = rec["screened_record_us"] / rec["plain_record_us"]
        rec["inactive_ratio"] = rec["inactive_us"] / rec["plain_us"]
        e.close()
        line = json.dumps(rec)
        print(line, flush=True)
        if args.out:
            with open(args.out, "a") as f:
                f.write(line + "\n")


if __name__ == "__main__":
    main()
