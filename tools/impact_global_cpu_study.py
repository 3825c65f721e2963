#!/usr/bin/env python3
"""tools/impact_global_cpu_study.py — the two CPU studies behind tests/test_gpu_impact_global.py, without a device: the
numpy restatements of the analyses, the oracle's steps, and the restated impacts.  The GPU stepper is the oracle bit
for bit, so this is the reference of those tests and not the code under test.  One JSON line per scenario.

  identity  seeds 1 .. 8, periodic and Dirichlet (value 0.5) sides, inflation 1 and 1.1: an ETKF
            (tests/etkf_restatement.py), six steps of members with one common (D, dt, vx, vy), the global impact
            (tests/impact_global_restatement.py): gap / scale of  sum_o J_o = mse_a - mse_b, and the localised total of
            the same capture beside it
  letkf     seeds 1 .. 8, the OSSE of tests/test_gpu_ensemble_impact.py with the LETKF at spacing 1 and 4
            (tests/letkf_restatement.py) and the localised impact (tests/impact_restatement.py): total / actual

  python tools/impact_global_cpu_study.py [--only identity|letkf] [--out F]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from __graft_entry__ import load_package  # noqa: E402
from oracle import cpu_oracle as oracle  # noqa: E402
import espace_restatement as espace  # noqa: E402
import etkf_restatement as etkf  # noqa: E402
import impact_global_restatement as ig  # noqa: E402
import impact_restatement as impact  # noqa: E402
import letkf_restatement as letkf  # noqa: E402
import obsnet_restatement as obsnet  # noqa: E402


def run(X, phys_of, sides, value, steps):
    """every member `steps` oracle steps on, each with its own (D, dt, vx, vy)"""
    nx, ny, dx, dy, _ = ig.GRID
    out = X.copy()
    for m in range(X.shape[0]):
        D, dt, vx, vy = phys_of(m)
        u = np.ascontiguousarray(out[m])
        oracle.run_single(u, dx, dy, D, vx, vy, dt, oracle.bc_codes(sides), steps, value)
        out[m] = u
    return out


def identity(pkg, seed, sides, value, lam):
    nx, ny, dx, dy, loc = ig.GRID
    X, i, j = ig.identity_members(seed, sides)
    y = ig.identity_values(X, i, j, seed)
    r = np.full(len(i), ig.OSSE_R)
    rho = pkg.ensemble_gc_table(dx, dy, loc, nx, ny)
    ly, lx = (rho.shape[0] - 1) // 2, (rho.shape[1] - 1) // 2
    order = etkf.plan_order(pkg.ensemble_assim_plan(i, j, lx, ly))
    hb, _ = obsnet.mv(X, 0, i, j)
    A, _, _ = etkf.obs_gram(X[1:, j, i], y, r, True, order)
    W, wbar, _, _, _ = etkf.etkf_weights(A, lam, pkg.sym_eigen)
    Xan = espace.transform(X, W, wbar, 0, True)
    cap = impact.capture(Xan, 0, i, j, None, y, hb, r)
    common = lambda m: ig.COMMON_PHYS  # noqa: E731
    Xa, Xb = run(Xan, common, sides, value, ig.OSSE_STEPS), run(X, common, sides, value, ig.OSSE_STEPS)
    total, actual, scale, rel = ig.identity_figures(Xa, Xb, cap, impact.impact_weight)
    w = impact.impact_weight(Xa[1:].mean(axis=0), Xb[1:].mean(axis=0), Xa[0])
    localised = impact.summary(impact.impact(Xa, cap, rho, i, j, w), cap.status)[2]
    return dict(study="identity", seed=seed, sides=sides, value=value, inflation=lam, total=total, actual=actual,
                scale=scale, gap_over_scale=rel, localised_total=localised)


def letkf_osse(pkg, seed, spacing):
    nx, ny, dx, dy, loc = ig.GRID
    X, i, j = ig.osse_members(seed)
    r = np.full(len(i), ig.OSSE_R)
    y, _ = obsnet.observe(X, 0, i, j, r, seed, 0, True)
    rho = pkg.ensemble_gc_table(dx, dy, loc, nx, ny)
    hb, _ = obsnet.mv(X, 0, i, j)
    eig = lambda C: pkg.sym_eigen(C, order="round_robin")  # noqa: E731
    Xan, _, _ = letkf.analysis(X, rho, i, j, None, y, r, 1.0, 0, spacing, eig)
    cap = impact.capture(Xan, 0, i, j, None, y, hb, r)
    phys = lambda m: ig.OSSE_PHYS[m % len(ig.OSSE_PHYS)]  # noqa: E731
    Xa, Xb = run(Xan, phys, "dddd", 0.5, ig.OSSE_STEPS), run(X, phys, "dddd", 0.5, ig.OSSE_STEPS)
    mean_a, mean_b, truth = Xa[1:].mean(axis=0), Xb[1:].mean(axis=0), Xa[0]
    w = impact.impact_weight(mean_a, mean_b, truth)
    J = impact.impact(Xa, cap, rho, i, j, w)
    used, beneficial, total = impact.summary(J, cap.status)
    actual = ig.mse(mean_a, truth) - ig.mse(mean_b, truth)
    return dict(study="letkf", seed=seed, spacing=spacing, total=float(total), actual=actual, ratio=float(total / actual),
                beneficial=beneficial, used=used)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", choices=("identity", "letkf"))
    ap.add_argument("--out", help="append the JSON lines to this file too")
    args = ap.parse_args()
    pkg = load_package()
    pkg.lib()
    recs = []
    if args.only != "letkf":
        for sides, value in ig.IDENTITY_SIDES:
            for lam in ig.IDENTITY_INFLATIONS:
                recs += [identity(pkg, seed, sides, value, lam) for seed in ig.SEEDS]
                print(json.dumps(recs[-1]), flush=True)
        worst = max(r["gap_over_scale"] for r in recs)
        print(json.dumps(dict(study="identity", largest_gap_over_scale=worst)), flush=True)
    if args.only != "identity":
        for s in (1, 4):
            rows = [letkf_osse(pkg, seed, s) for seed in ig.SEEDS]
            recs += rows
            print(json.dumps(dict(study="letkf", spacing=s, ratio_min=min(r["ratio"] for r in rows),
                                  ratio_max=max(r["ratio"] for r in rows),
                                  actual_max=max(r["actual"] for r in rows), total_max=max(r["total"] for r in rows),
                                  beneficial_min=min(r["beneficial"] for r in rows))), flush=True)
    if args.out:
        with open(args.out, "a") as f:
            for r in recs:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
