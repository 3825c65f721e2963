#!/usr/bin/env python3
"""tools/ensemble_etkf_bench.py — cost of the ETKF (csim_ensemble_obs_gram, csim_etkf_weights,
csim_ensemble_assimilate_etkf), one JSON line per configuration.  The method of tools/ensemble_gram_bench.py: ten calls
per timed region, five regions, the median and the spread (max - min) / median reported.

For B members of n x n (all of them forecast members) and a network of nobs point observations at distinct random cells:
  obs_gram_us         csim_ensemble_obs_gram, A only (two kernels, the copy of A and one stream sync);
  etkf_weights_us     csim_etkf_weights alone on that matrix (host: the eigensolver and two small products);
  assimilate_etkf_us  csim_ensemble_assimilate_etkf, then a sync (obs_gram, the weights, transform);
and two yardsticks measured in the same process:
  assimilate_network_us   csim_ensemble_assimilate_network on the same network, then a sync: the serial filter;
  gram_us                 csim_ensemble_gram, centered, on an ensemble of B members whose interior has as many cells as
                          the network has observations: the same pair arithmetic with contiguous staging.
Ratios: obs_gram_over_gram, assimilate_etkf_over_network.  Before timing, A is checked against numpy within 1e-10
relative and symmetric bit for bit.

  python tools/ensemble_etkf_bench.py --config 64x512x1024 --config 64x512x16384 --config 256x256x1024 [--out FILE]
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

REGIONS = 5


def timed(fn, calls):
    """(median, spread) of the time per call over REGIONS regions of `calls` calls"""
    out = []
    for _ in range(REGIONS):
        t0 = time.perf_counter()
        for _ in range(calls):
            fn()
        out.append((time.perf_counter() - t0) / calls)
    med = statistics.median(out)
    return med, (max(out) - min(out)) / med


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", action="append", default=[], help="BxNxO: B members of N x N, O observations")
    ap.add_argument("--calls", type=int, default=10, help="device calls per timed region")
    ap.add_argument("--only", choices=["obs_gram", "assimilate_etkf"],
                    help="only --calls calls of this one (for a profiler or counter run)")
    ap.add_argument("--obs-gram-form", type=int, default=0)
    ap.add_argument("--loc", type=float, default=4.0, help="localisation length of the network (the serial yardstick)")
    ap.add_argument("--out", help="append the JSON lines to this file too")
    args = ap.parse_args()
    pkg = load_package()
    pkg.set_device(0)
    lib = pkg.lib()

    def ok(rc):
        if rc:
            raise SystemExit(lib.csim_last_error().decode())

    for cfg in args.config or ["64x512x1024", "64x512x16384", "256x256x1024"]:
        B, n, nobs = (int(v) for v in cfg.split("x"))
        rng = np.random.default_rng(B * 7 + n + nobs)
        X = 1.0 + rng.random((B, n + 2, n + 2))
        e = pkg.Ensemble(B, n, n, 1.0, 1.0, [0, 0, 0, 0])
        e.upload_all(X)
        e.set_option("obs_gram_form", args.obs_gram_form)
        cells = rng.permutation(n * n)[:nobs]
        i, j = (cells % n + 1).astype(np.int32), (cells // n + 1).astype(np.int32)
        r = rng.uniform(0.5, 2.0, nobs)
        y = 1.5 + 0.3 * rng.standard_normal(nobs)
        net = e.obs_network(i, j, r, args.loc)
        net.set_values(y)

        def obs_gram():
            return e.obs_gram(net)

        def assimilate_etkf():
            ok(lib.csim_ensemble_assimilate_etkf(e._h, net._h, 1.0, -1, 0, 0.0))
            ok(lib.csim_ensemble_sync(e._h))

        if args.only:
            for _ in range(args.calls):
                {"obs_gram": obs_gram, "assimilate_etkf": assimilate_etkf}[args.only]()
            e.close()
            continue

        def assimilate_network():
            ok(lib.csim_ensemble_assimilate_network(e._h, net._h, 1.0, -1, 0))
            ok(lib.csim_ensemble_sync(e._h))

        A = obs_gram().A
        H = X[:, j, i]
        hb = H.mean(axis=0)
        Z = np.vstack([H - hb, (y - hb)[None]]) / np.sqrt(r)
        want = Z @ Z.T
        if not (np.array_equal(A.view(np.int64), A.T.copy().view(np.int64))
                and np.abs(A - want).max() <= 1e-10 * np.abs(want).max()):
            raise SystemExit(f"{cfg}: the observation-space Gram matrix differs from numpy")

        # the yardstick of the pair arithmetic: as many contiguous cells as observations
        side = max(1, int(round(nobs ** 0.5)))
        rows = -(-nobs // side)
        g = pkg.Ensemble(B, side, rows, 1.0, 1.0, [0, 0, 0, 0])
        g.upload_all(1.0 + rng.random((B, rows + 2, side + 2)))

        rec = dict(config=cfg, members=B, n=n, nobs=nobs, loc=args.loc, nlevels=net.info.nlevels, calls=args.calls,
                   regions=REGIONS, obs_gram_form=args.obs_gram_form, gram_cells=side * rows)
        for name, fn in (("obs_gram", obs_gram), ("gram", g.gram), ("etkf_weights", lambda: pkg.etkf_weights(A)),
                         ("assimilate_etkf", assimilate_etkf), ("assimilate_network", assimilate_network)):
            if name == "assimilate_network":
                e.upload_all(X)  # both analyses start from the same members
            fn()
            med, spread = timed(fn, args.calls)
            rec[name + "_us"], rec[name + "_spread"] = med * 1e6, spread
        rec["obs_gram_over_gram"] = rec["obs_gram_us"] / rec["gram_us"]
        rec["assimilate_etkf_over_network"] = rec["assimilate_etkf_us"] / rec["assimilate_network_us"]
        e.close(), g.close()
        line = json.dumps(rec)
        print(line, flush=True)
        if args.out:
            with open(args.out, "a") as f:
                f.write(line + "\n")


if __name__ == "__main__":
    main()
