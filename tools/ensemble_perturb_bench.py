#!/usr/bin/env python3
"""tools/ensemble_perturb_bench.py — cost of the ensemble perturbation (csim_ensemble_perturb), one JSON line per
configuration and (radius, centered).

For B members of n x n (Dirichlet on all sides, unit spacing) and corr_len chosen so that the tap radius is R:
  call_us         one csim_ensemble_perturb followed by a stream sync (one launch), the mean over `--calls` calls,
                  median of three regions; a new `draw` every call;
  host_s          what the call replaces, on the same machine in the same run: numpy standard_normal of the same shape
                  (white noise: the host path does not even smooth) + upload_all, wall time, once per configuration;
  host_over_call  host_s / call time;
  floor_us        one read and one write of the B interior fields (16 B n n bytes) at `--hbm-gbps`, the rate
                  tools/membench reports for a copy;
  floor_fraction  floor_us / call_us.
Kernel times and counters come from rocprofv3 runs of `--only-perturb` (only `--calls` perturbations, no host path);
each GPU step of such a session runs under its own `timeout`.

  python tools/ensemble_perturb_bench.py --config 256x256 --config 64x512 --config 64x1024 [--out F]
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

CORR = {0: 0.0, 4: 2.25, 16: 8.25}  # corr_len with (double)a < 2 corr_len for a <= R only


def timed(fn, regions=3):
    out = []
    for _ in range(regions):
        t0 = time.perf_counter()
        fn()
        out.append(time.perf_counter() - t0)
    return statistics.median(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", action="append", default=[], help="BxN")
    ap.add_argument("--radius", action="append", type=int, default=[], choices=sorted(CORR))
    ap.add_argument("--calls", type=int, default=10, help="perturbations per timed region")
    ap.add_argument("--hbm-gbps", type=float, default=0.0, help="copy rate of tools/membench (0: no floor)")
    ap.add_argument("--only-perturb", action="store_true", help="only --calls perturbations each (profiler)")
    ap.add_argument("--no-host", action="store_true", help="skip the host path")
    ap.add_argument("--out", help="append the JSON lines to this file too")
    args = ap.parse_args()
    pkg = load_package()
    pkg.set_device(0)
    for cfg in args.config or ["256x256", "64x512", "64x1024"]:
        B, n = (int(v) for v in cfg.split("x"))
        e = pkg.Ensemble(B, n, n, 1.0, 1.0, [0, 0, 0, 0])
        host_s = None
        if not (args.no_host or args.only_perturb):
            rng = np.random.default_rng(B + n)
            t0 = time.perf_counter()
            e.upload_all(rng.standard_normal((B, n + 2, n + 2)))
            e.sync()
            host_s = time.perf_counter() - t0
        for R in args.radius or sorted(CORR):
            assert len(pkg.ensemble_perturb_taps(1.0, CORR[R], n)) == 2 * R + 1
            for centered in (False, True):
                draw = [0]

                def call():
                    for _ in range(args.calls):
                        draw[0] += 1
                        e.perturb(0.01, CORR[R], 1234, draw[0], centered=centered)
                        e.sync()
                call()
                if args.only_perturb:
                    continue
                t = timed(call) / args.calls
                rec = dict(config=cfg, members=B, n=n, radius=R, centered=int(centered), calls=args.calls,
                           call_us=t * 1e6, fields_per_s=B / t)
                if host_s is not None:
                    rec.update(host_s=host_s, host_over_call=host_s / t)
                if args.hbm_gbps > 0:
                    floor = 16.0 * B * n * n / (args.hbm_gbps * 1e9)
                    rec.update(hbm_gbps=args.hbm_gbps, floor_us=floor * 1e6, floor_fraction=floor / t)
                line = json.dumps(rec)
                print(line, flush=True)
                if args.out:
                    with open(args.out, "a") as f:
                        f.write(line + "\n")
        e.close()


if __name__ == "__main__":
    main()
