#!/usr/bin/env python3
"""tools/ensemble_bench.py — rate of the batched stepper against the alternatives, one JSON line per configuration.

For B members of n x n (Dirichlet on all sides, the same physics for every member) it times, in Mcell-updates/s:
  ensemble   one csim_ensemble, `--steps` steps of every member per timed region;
  separate   the same members as B single-rank Steppers run one after another, one sync at the end;
  single     one Stepper on a square grid with the same total number of cells (e.g. 64 x 512^2 -> 4096^2).
Each rate is the median of three timed regions, each after keep_warm (as bench.py does).  Before timing, the
ensemble's checksums of a sampled subset of members are checked against the oracle.

  python tools/ensemble_bench.py --config 256x256 --config 64x512 [--physics adv|diff] [--steps 100]
"""
import argparse
import json
import math
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from __graft_entry__ import load_package  # noqa: E402
from oracle import cpu_oracle as ora  # noqa: E402

PHYSICS = {"adv": dict(D=0.05, vx=0.5, vy=0.25), "diff": dict(D=0.05, vx=0.0, vy=0.0)}
WARM_S = 0.3


def timed(fn, warm, regions=3):
    out = []
    for _ in range(regions):
        warm()
        t0 = time.perf_counter()
        fn()
        out.append(time.perf_counter() - t0)
    return statistics.median(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", action="append", default=[], help="BxN: B members of N x N")
    ap.add_argument("--physics", default="adv", choices=sorted(PHYSICS))
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--check", type=int, default=4, help="members checked against the oracle before timing")
    ap.add_argument("--no-separate", action="store_true")
    args = ap.parse_args()
    pkg = load_package()
    pkg.set_device(0)
    ph = PHYSICS[args.physics]
    D, vx, vy = ph["D"], ph["vx"], ph["vy"]
    dt = min(0.1, pkg.safe_dt(1.0, 1.0, vx, vy, D))
    bc = [0, 0, 0, 0]
    for cfg in args.config or ["256x256", "64x512"]:
        B, n = (int(v) for v in cfg.split("x"))
        K = args.steps
        rng = np.random.default_rng(B * 7 + n)
        u0 = np.zeros((B, n + 2, n + 2))
        u0[:, 1:-1, 1:-1] = rng.random((B, n, n))
        side = int(round(math.sqrt(B) * n))
        big = pkg.Stepper.single(side, side, 1.0, 1.0, bc)
        big.init_gaussian()

        def warm():
            big.keep_warm(D, dt, vx, vy, WARM_S)

        e = pkg.Ensemble(B, n, n, 1.0, 1.0, bc)
        e.upload_all(u0)
        e.set_physics(D, dt, vx, vy)
        e.run(K)
        sums = e.checksums()
        picks = sorted(set(np.linspace(0, B - 1, min(args.check, B)).astype(int).tolist()))
        for k in picks:
            w = u0[k].copy()
            ora.run_single(w, 1.0, 1.0, D, vx, vy, dt, bc, K)
            if sums[k] != pkg.checksum_host(w[1:-1, 1:-1]):
                raise SystemExit(f"{cfg}: member {k} differs from the oracle")

        def run_ens():
            e.run(K)
            e.sync()
        t_ens = timed(run_ens, warm)
        rec = dict(config=cfg, members=B, n=n, physics=args.physics, D=D, vx=vx, vy=vy, dt=dt, steps=K,
                   depth=e.get_option("depth_used"), checked_members=picks,
                   ensemble_mcups=B * n * n * K / t_ens / 1e6)
        e.close()
        if not args.no_separate:
            sts = []
            for k in range(B):
                s = pkg.Stepper.single(n, n, 1.0, 1.0, bc)
                s.upload(u0[k])
                sts.append(s)

            def run_sep():
                for s in sts:
                    s.run(D, dt, vx, vy, K)
                for s in sts:
                    s.sync()
            run_sep()
            t_sep = timed(run_sep, warm)
            for s in sts:
                s.close()
            rec["separate_mcups"] = B * n * n * K / t_sep / 1e6
            rec["ensemble_over_separate"] = rec["ensemble_mcups"] / rec["separate_mcups"]

        def run_big():
            big.run(D, dt, vx, vy, K)
            big.sync()
        run_big()
        t_big = timed(run_big, warm)
        rec["single_side"] = side
        rec["single_mcups"] = side * side * K / t_big / 1e6
        rec["ensemble_over_single"] = rec["ensemble_mcups"] / rec["single_mcups"]
        big.close()
        print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
