#!/usr/bin/env python3
"""tools/ensemble_impact_global_bench.py — what the ensemble-space dot and the global forecast impact cost
(csim_ensemble_dot, csim_ensemble_obs_impact_global), one JSON line per configuration, in the style of
tools/ensemble_impact_bench.py: the mean over `--calls` calls that each start on an idle stream and end with a stream
sync, over `--regions` regions after a warm-up region; median, and the least and the largest region as the spread.

  --dot BxN      B members of n x n, all of them forecast members:
    stats_us       csim_ensemble_stats with every output NULL: the project's measured single read of the members
    gram_us        csim_ensemble_gram, centered
    dot1_us, dot16_us   csim_ensemble_dot with K = 1 and K = 16, centered: the check and the packing of the fields'
                   interiors on the host, their copy to the device, two kernels, the copy of M x K values back
    stage1_us, stage16_us   the host part alone, measured as the same call on an ensemble of one member of the same
                   grid, whose kernels read 1 / B of the members
  --impact BxN:OBS   the networks of tools/ensemble_impact_bench.py (member 0 the truth, M = B - 1), a capture after a
                 recorded ETKF:
    impact_us          csim_ensemble_obs_impact, the localised call
    impact_global_us   csim_ensemble_obs_impact_global
  --only NAME    only --calls calls of gram, dot1, dot16, impact or impact_global on the first configuration, for a
                 profiler run that times the kernels apart

  python tools/ensemble_impact_global_bench.py --dot 64x1024 --impact 64x512:lattice16 [--out F]
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


def measure(e, call, calls, regions):
    def region():
        total = 0.0
        for _ in range(calls):
            e.sync()
            t0 = time.perf_counter()
            call()
            e.sync()
            total += time.perf_counter() - t0
        return total / calls * 1e6
    region()
    t = sorted(region() for _ in range(regions))
    return statistics.median(t), t[0], t[-1]


def put(rec, key, m):
    rec[key + "_us"], rec[key + "_min_us"], rec[key + "_max_us"] = m


def members(B, n, rng):
    """B members of (n+2) x (n+2) around 3, filled member by member"""
    X = np.empty((B, n + 2, n + 2))
    for m in range(B):
        X[m] = 3.0 + rng.standard_normal((n + 2, n + 2))
    return X


def bench_dot(pkg, cfg, args):
    B, n = (int(v) for v in cfg.split("x"))
    rng = np.random.default_rng(B * 11 + n)
    e = pkg.Ensemble(B, n, n, 1.0, 1.0, [0, 0, 0, 0])
    e.upload_all(members(B, n, rng))
    one = pkg.Ensemble(1, n, n, 1.0, 1.0, [0, 0, 0, 0])
    F = rng.standard_normal((16, n + 2, n + 2))
    f1 = np.ascontiguousarray(F[:1])
    first = e.dot(F)
    if first.tobytes() != e.dot(F).tobytes() or first[:, :1].tobytes() != e.dot(f1).tobytes():
        raise SystemExit(f"{cfg}: two evaluations of dot differ")
    if not np.isfinite(first).all():
        raise SystemExit(f"{cfg}: dot is not finite")
    stats_call = lambda: pkg.lib().csim_ensemble_stats(e._h, 1, None, None, None, None)  # noqa: E731
    calls = dict(stats=stats_call, gram=lambda: e.gram(), dot1=lambda: e.dot(f1), dot16=lambda: e.dot(F),
                 stage1=lambda: one.dot(f1), stage16=lambda: one.dot(F))
    if args.only:
        for _ in range(args.calls):
            calls[args.only]()
        return None
    rec = dict(kind="dot", config=cfg, members=B, n=n, calls=args.calls, regions=args.regions)
    for key, call in calls.items():
        put(rec, key, measure(e, call, args.calls, args.regions))
    rec["dot1_over_gram"] = rec["dot1_us"] / rec["gram_us"]
    rec["dot1_less_stage_over_gram"] = (rec["dot1_us"] - rec["stage1_us"]) / rec["gram_us"]
    rec["dot1_less_stage_over_stats"] = (rec["dot1_us"] - rec["stage1_us"]) / rec["stats_us"]
    rec["dot16_less_stage_over_stats"] = (rec["dot16_us"] - rec["stage16_us"]) / rec["stats_us"]
    e.close(), one.close()
    return rec


def bench_impact(pkg, cfg, args):
    size, kind = cfg.split(":")
    B, n = (int(v) for v in size.split("x"))
    rng = np.random.default_rng(B * 7 + n)
    i, j = observations(kind, n, rng)
    nobs = len(i)
    y = 3.0 + rng.standard_normal(nobs)
    w = rng.standard_normal((n + 2, n + 2))
    e = pkg.Ensemble(B, n, n, 1.0, 1.0, [0, 0, 0, 0])
    net = e.obs_network(i, j, R, args.loc, log_cycles=1)
    net.set_values(y)
    info = net.info
    e.upload_all(members(B, n, rng))
    e.assimilate_etkf(net, truth_member=0, record=True, device=True)
    net.impact_capture(truth_member=0)
    first, second = e.obs_impact_global(net, w), e.obs_impact_global(net, w)
    if first.impact.tobytes() != second.impact.tobytes() or first.summary != second.summary:
        raise SystemExit(f"{cfg}: two evaluations of one capture differ")
    if not np.isfinite(first.impact).all() or first.summary.used != nobs:
        raise SystemExit(f"{cfg}: the impact is not finite")
    calls = dict(impact=lambda: e.obs_impact(net, w), impact_global=lambda: e.obs_impact_global(net, w))
    if args.only:
        for _ in range(args.calls):
            calls[args.only]()
        return None
    rec = dict(kind="impact", config=cfg, members=B, n=n, nobs=nobs, loc=args.loc,
               window=(2 * info.lx + 1) * (2 * info.ly + 1), calls=args.calls, regions=args.regions,
               total_global=first.summary.total, total_localised=e.obs_impact(net, w).summary.total)
    for key, call in calls.items():
        put(rec, key, measure(e, call, args.calls, args.regions))
    rec["global_over_localised"] = rec["impact_global_us"] / rec["impact_us"]
    e.close()
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dot", action="append", default=[], help="BxN")
    ap.add_argument("--impact", action="append", default=[], help="BxN:OBS, OBS = latticeS or randomK")
    ap.add_argument("--loc", type=float, default=8.0)
    ap.add_argument("--calls", type=int, default=10, help="calls per timed region")
    ap.add_argument("--regions", type=int, default=5, help="timed regions per number, after one warm-up region")
    ap.add_argument("--only", choices=("stats", "gram", "dot1", "dot16", "impact", "impact_global"))
    ap.add_argument("--out", help="append the JSON lines to this file too")
    args = ap.parse_args()
    pkg = load_package()
    pkg.set_device(0)
    jobs = [(bench_dot, c) for c in args.dot] + [(bench_impact, c) for c in args.impact]
    for fn, cfg in jobs[:1] if args.only else jobs:
        rec = fn(pkg, cfg, args)
        if rec is None:
            continue
        line = json.dumps(rec)
        print(line, flush=True)
        if args.out:
            with open(args.out, "a") as f:
                f.write(line + "\n")


if __name__ == "__main__":
    main()
