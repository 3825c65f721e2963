#!/usr/bin/env python3
"""tools/ensemble_gram_bench.py — cost of the ensemble-space calls (csim_ensemble_gram, _project, _transform, _eofs),
one JSON line per configuration.

For B members of n x n (all of them forecast members), five timed regions each, the median and the spread
(max - min) / median reported:
  stats_us       csim_ensemble_stats with every output NULL on the same ensemble in the same process: the project's
                 measured single read of the members, the yardstick of a pass over them;
  gram_us        csim_ensemble_gram, centered (two kernels, the copy of G and one stream sync);
  project_us     csim_ensemble_project with K = 4, centered (the kernel and the copy of four fields to the host);
  transform_us   csim_ensemble_transform with W = I + small, centered, with wbar, then a sync;
  eofs_us        csim_ensemble_eofs with four modes and patterns (gram, the host eigensolver, project);
  sym_eigen_us   csim_sym_eigen alone on that ensemble's Gram matrix (host);
  host_gram_us   what a user does without these calls: download_all() and numpy P @ P.T of the centered interior;
  host_transform_us   download_all(), numpy einsum, upload_all().
Ratios: gram_over_stats, and host_gram_over_gram / host_transform_over_transform (how much the round trip costs more).
Before timing, G is checked against numpy within 1e-10 relative and symmetric bit for bit.

  python tools/ensemble_gram_bench.py --config 64x1024 --config 64x512 --config 256x256 --config 128x512 [--out FILE]
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
    ap.add_argument("--config", action="append", default=[], help="BxN: B members of N x N")
    ap.add_argument("--calls", type=int, default=10, help="device calls per timed region")
    ap.add_argument("--only", choices=["gram", "project", "transform"],
                    help="only --calls calls of this one (for a profiler or counter run)")
    ap.add_argument("--gram-form", type=int, default=0)
    ap.add_argument("--project-form", type=int, default=0)
    ap.add_argument("--no-host", action="store_true", help="skip the host round trips")
    ap.add_argument("--out", help="append the JSON lines to this file too")
    args = ap.parse_args()
    pkg = load_package()
    pkg.set_device(0)
    lib, C = pkg.lib(), pkg.C
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))  # noqa: E731

    def ok(rc):
        if rc:
            raise SystemExit(lib.csim_last_error().decode())

    for cfg in args.config or ["64x1024", "64x512", "256x256", "128x512"]:
        B, n = (int(v) for v in cfg.split("x"))
        rng = np.random.default_rng(B * 7 + n)
        e = pkg.Ensemble(B, n, n, 1.0, 1.0, [0, 0, 0, 0])
        e.upload_all(1.0 + rng.random((B, n + 2, n + 2)))
        e.set_option("gram_form", args.gram_form)
        e.set_option("project_form", args.project_form)
        G, out4 = np.empty((B, B)), np.empty((4, n + 2, n + 2))
        W4 = rng.standard_normal((B, 4))
        T = np.eye(B) + 1e-3 * rng.standard_normal((B, B))
        wbar = 1e-3 * rng.standard_normal(B)
        lam, pcs = np.empty(4), np.empty((B, 4))

        def gram():
            ok(lib.csim_ensemble_gram(e._h, -1, 1, dp(G)))

        def project():
            ok(lib.csim_ensemble_project(e._h, -1, 1, 4, dp(W4), dp(out4)))

        def transform():
            ok(lib.csim_ensemble_transform(e._h, -1, 1, dp(T), dp(wbar)))
            ok(lib.csim_ensemble_sync(e._h))

        if args.only:
            for _ in range(args.calls):
                {"gram": gram, "project": project, "transform": transform}[args.only]()
            e.close()
            continue

        def stats():
            ok(lib.csim_ensemble_stats(e._h, 1, None, None, None, None))

        def eofs():
            ok(lib.csim_ensemble_eofs(e._h, -1, 4, dp(lam), dp(pcs), dp(out4), None))

        def host_gram():
            a = e.download_all()[:, 1:-1, 1:-1].reshape(B, -1)
            p = a - a.mean(axis=0)
            return p @ p.T

        def host_transform():
            a = e.download_all()
            m = a.mean(axis=0)
            p = a - m
            a[:, 1:-1, 1:-1] = ((m + np.einsum("k,kji->ji", wbar, p))[None]
                                + np.einsum("kr,kji->rji", T, p, optimize=True))[:, 1:-1, 1:-1]
            e.upload_all(a)

        gram()
        want = host_gram()
        if not (np.array_equal(G.view(np.int64), G.T.copy().view(np.int64))
                and np.abs(G - want).max() <= 1e-10 * np.abs(want).max()):
            raise SystemExit(f"{cfg}: the Gram matrix differs from numpy")
        rec = dict(config=cfg, members=B, n=n, calls=args.calls, regions=REGIONS,
                   gram_form=args.gram_form, project_form=args.project_form)
        for name, fn, calls in (("stats", stats, args.calls), ("gram", gram, args.calls),
                                ("project", project, args.calls), ("eofs", eofs, max(1, args.calls // 5)),
                                ("sym_eigen", lambda: pkg.sym_eigen(G), max(1, args.calls // 5))):
            fn()
            med, spread = timed(fn, calls)
            rec[name + "_us"], rec[name + "_spread"] = med * 1e6, spread
        if not args.no_host:
            med, spread = timed(host_gram, 1)
            rec["host_gram_us"], rec["host_gram_spread"] = med * 1e6, spread
            rec["host_gram_over_gram"] = rec["host_gram_us"] / rec["gram_us"]
        # the transforms last: they change the members (T is near the identity, so they stay finite)
        transform()
        med, spread = timed(transform, args.calls)
        rec["transform_us"], rec["transform_spread"] = med * 1e6, spread
        if not args.no_host:
            med, spread = timed(host_transform, 1)
            rec["host_transform_us"], rec["host_transform_spread"] = med * 1e6, spread
            rec["host_transform_over_transform"] = rec["host_transform_us"] / rec["transform_us"]
        rec["gram_over_stats"] = rec["gram_us"] / rec["stats_us"]
        rec["project_over_stats"] = rec["project_us"] / rec["stats_us"]
        rec["transform_over_stats"] = rec["transform_us"] / rec["stats_us"]
        e.close()
        line = json.dumps(rec)
        print(line, flush=True)
        if args.out:
            with open(args.out, "a") as f:
                f.write(line + "\n")


if __name__ == "__main__":
    main()
