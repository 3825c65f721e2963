#!/usr/bin/env python3
"""tools/ensemble_relax_bench.py — cost of the relaxation inflation (csim_ensemble_prior_capture / csim_ensemble_relax),
one JSON line per configuration.

For B members of n x n (Dirichlet on all sides, the same advection physics for every member, M = B forecast members),
after the result has been checked bit for bit against tests/relax_restatement.py at that size (both modes), each call
followed by a stream sync, the mean over `--calls` calls, median of three regions:
  capture_us       prior_capture("spread")                       (k_relax_capture)
  stats_us         stats_begin(); stats_wait() of the same ensemble (the statistics kernel: same reads, four stores)
  inflate_us       assimilate(nobs = 0, inflation = 1.1)          (k_assim_inflate: the yardstick of the dense relax)
  relax_dense_us   relax(0.1) after an analysis = prior x 0.5 everywhere: every cell is written in every call
  relax_sparse_us  relax(0.1) after an analysis of a 16-cell lattice with c = 2 cells: most cells have f == 0
  capture_pert_us  prior_capture("pert")                          (one device-to-device copy)
  relax_pert_us    relax(0.1, "pert"); pert_gbps = 24 M n^2 bytes (x and xb read, x written) over it
  cycle_us         `--loops` x (capture; assimilate; relax; run(20)) against plain_us: `--loops` x (assimilate;
                   run(20)), then one sync, per iteration; observations as the configuration says, c = `--loc` cells
  host_s           the host path: download_all, the restatement vectorised (mean / std over axis 0), upload_all
Kernel times come from a rocprofv3 --kernel-trace --stats run of `--only-kernels` (only `--calls` calls of each kernel,
no check, no host path).

  python tools/ensemble_relax_bench.py --config 64x512:lattice16 --config 64x1024:lattice16 \
      --config 256x256:random1024 [--out F]
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
sys.path.insert(0, os.path.join(ROOT, "tests"))
from __graft_entry__ import load_package  # noqa: E402
import relax_restatement as ref  # noqa: E402

D, VX, VY = 0.05, 0.5, 0.25
RUN = 20
R = 0.5


def timed(fn, regions=3):
    out = []
    for _ in range(regions):
        t0 = time.perf_counter()
        fn()
        out.append(time.perf_counter() - t0)
    return statistics.median(out)


def observations(kind, n, rng):
    if kind.startswith("lattice"):
        s = int(kind[len("lattice"):])
        g = np.arange(s // 2, n + 1, s)
        I, J = np.meshgrid(g, g)
        i, j = I.ravel(), J.ravel()
    else:
        k = int(kind[len("random"):])
        i, j = rng.integers(1, n + 1, k), rng.integers(1, n + 1, k)
    return i.astype(np.int32), j.astype(np.int32), rng.standard_normal(len(i))


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.int64), b.view(np.int64))


def host_relax(X, sb, alpha):
    """the RTPS relaxation the way a user would write it in numpy (not bit for bit the definition)"""
    m = X[:, 1:-1, 1:-1].mean(axis=0)
    sa = X[:, 1:-1, 1:-1].std(axis=0, ddof=1)
    f = np.where(sa > 0, alpha * (sb - sa) / np.where(sa > 0, sa, 1.0), 0.0)
    X[:, 1:-1, 1:-1] += f * (X[:, 1:-1, 1:-1] - m)
    return X


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", action="append", default=[], help="BxN:OBS, OBS = latticeS or randomK")
    ap.add_argument("--loc", type=float, default=8.0)
    ap.add_argument("--calls", type=int, default=20, help="calls per timed region")
    ap.add_argument("--loops", type=int, default=10, help="cycle iterations per timed region")
    ap.add_argument("--only-kernels", action="store_true", help="only --calls calls of each kernel (profiler)")
    ap.add_argument("--no-host", action="store_true", help="skip the host path")
    ap.add_argument("--out", help="append the JSON lines to this file too")
    args = ap.parse_args()
    pkg = load_package()
    pkg.set_device(0)
    dt = min(0.1, pkg.safe_dt(1.0, 1.0, VX, VY, D))
    for cfg in args.config or ["64x512:lattice16", "64x1024:lattice16", "256x256:random1024"]:
        size, kind = cfg.split(":")
        B, n = (int(v) for v in size.split("x"))
        rng = np.random.default_rng(B * 7 + n)
        i, j, y = observations(kind, n, rng)
        si, sj, sy = observations("lattice16", n, rng)
        e = pkg.Ensemble(B, n, n, 1.0, 1.0, [0, 0, 0, 0])
        X = rng.standard_normal((B, n + 2, n + 2))
        e.upload_all(X)
        e.set_physics(D, dt, VX, VY)
        rec = dict(config=cfg, members=B, n=n, nobs=len(i), loc=args.loc, calls=args.calls)

        if not args.only_kernels:
            A = 0.5 * X
            for mode, code in (("spread", ref.SPREAD), ("pert", ref.PERT)):
                e.upload_all(X)
                e.prior_capture(mode)
                e.upload_all(A)
                e.relax(0.5, mode)
                want, _ = ref.relax(A, ref.capture(X, code), code, 0.5)
                if not same_bits(e.download_all(), want):
                    raise SystemExit(f"{cfg}: relax({mode}) differs from the numpy restatement")
            del want
            if not args.no_host:
                sb = X[:, 1:-1, 1:-1].std(axis=0, ddof=1)
                e.upload_all(A)
                t0 = time.perf_counter()
                e.upload_all(host_relax(e.download_all(), sb, 0.5))
                rec["host_s"] = time.perf_counter() - t0
            del A

        def repeat(fn):
            def body():
                for _ in range(args.calls):
                    fn()
                    e.sync()
            body()  # warm-up; with --only-kernels the profiled calls
            return None if args.only_kernels else timed(body) / args.calls * 1e6

        def stats():
            e.stats_begin()
            e.stats_wait()

        e.upload_all(X)
        rec["capture_us"] = repeat(lambda: e.prior_capture("spread"))
        rec["stats_us"] = repeat(stats)
        rec["inflate_us"] = repeat(lambda: e.assimilate([], [], [], R, args.loc, inflation=1.1, diagnostics=False))
        e.upload_all(X)
        e.prior_capture("spread")
        # the analysis; every call gives back a tenth of what is left, so f stays far from 0 over all timed calls
        e.upload_all(0.5 * X)
        rec["relax_dense_us"] = repeat(lambda: e.relax(0.1))
        e.upload_all(X)
        e.prior_capture("spread")
        e.assimilate(si, sj, sy, R, 2.0, diagnostics=False)
        rec["relax_sparse_us"] = repeat(lambda: e.relax(0.1))
        e.upload_all(X)
        rec["capture_pert_us"] = repeat(lambda: e.prior_capture("pert"))
        e.upload_all(0.5 * X)
        rec["relax_pert_us"] = repeat(lambda: e.relax(0.1, "pert"))
        if args.only_kernels:
            e.close()
            continue
        rec["pert_gbps"] = 24.0 * B * n * n / rec["relax_pert_us"] / 1e3
        rec["dense_gbps"] = 16.0 * B * n * n / rec["relax_dense_us"] / 1e3
        rec["dense_over_inflate"] = rec["relax_dense_us"] / rec["inflate_us"]
        rec["capture_over_stats"] = rec["capture_us"] / rec["stats_us"]
        rec["sparse_over_dense"] = rec["relax_sparse_us"] / rec["relax_dense_us"]

        def cycle():
            for _ in range(args.loops):
                e.prior_capture("spread")
                e.assimilate(i, j, y, R, args.loc, diagnostics=False)
                e.relax(0.5)
                e.run(RUN)
            e.sync()

        def plain():
            for _ in range(args.loops):
                e.assimilate(i, j, y, R, args.loc, diagnostics=False)
                e.run(RUN)
            e.sync()
        e.upload_all(X)
        cycle()
        plain()
        t_cycle, t_plain = timed(cycle) / args.loops, timed(plain) / args.loops
        rec.update(cycle_us=t_cycle * 1e6, plain_us=t_plain * 1e6, relax_adds_us=(t_cycle - t_plain) * 1e6)
        if "host_s" in rec:
            rec["host_over_relax"] = rec["host_s"] / ((rec["capture_us"] + rec["relax_dense_us"]) * 1e-6)
        e.close()
        line = json.dumps(rec)
        print(line, flush=True)
        if args.out:
            with open(args.out, "a") as f:
                f.write(line + "\n")


if __name__ == "__main__":
    main()
