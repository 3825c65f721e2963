#!/usr/bin/env python3
"""tools/ensemble_etkf_device_bench.py — cost of the device ETKF (csim_sym_eigen_batch_gpu,
csim_ensemble_assimilate_etkf_device) beside the host path it stands in for, one JSON line per configuration.  The method
of tools/ensemble_etkf_bench.py: ten calls per timed region, five regions, the median and the spread (max - min) / median.

Lines of kind "eigen", per n: the public call on one matrix (which creates and frees its stream and buffer and copies the
matrix in and the result out), the host solver in both orders on the same Gram matrix, and with --batch the same call on a
batch of different matrices with its rate in matrices per second against batch x the single call.
Lines of kind "analysis", for B members of n x n and nobs point observations at distinct random cells:
  etkf_weights_us          csim_etkf_weights on the network's matrix: the host path's eigensolver and products;
  assimilate_etkf_us       csim_ensemble_assimilate_etkf, then a sync: the host path;
  device_us                csim_ensemble_assimilate_etkf_device, then a sync;
  device_enqueue_us        the host time of that call alone, the sync outside the timed region;
  obs_gram_us              csim_ensemble_obs_gram (two kernels, a copy, a sync): what both paths share.
With --only NAME the program makes --calls calls of that one and exits, for a profiler's kernel trace or a counter run.

  python tools/ensemble_etkf_device_bench.py [--config 64x512x1024 ...] [--eigen 64,128,256] [--batch 256x64] [--out FILE]
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


def timed(fn, calls, after=None):
    """(median, spread) of the time per call over REGIONS regions of `calls` calls; after() runs outside the timing"""
    out = []
    for _ in range(REGIONS):
        t0 = time.perf_counter()
        for _ in range(calls):
            fn()
        out.append((time.perf_counter() - t0) / calls)
        if after:
            after()
    med = statistics.median(out)
    return med, (max(out) - min(out)) / med


def gram(n, seed):
    rng = np.random.default_rng([seed, n])
    B = rng.standard_normal((n, n + 3))
    return B @ B.T


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", action="append", default=[], help="BxNxO: B members of N x N, O observations")
    ap.add_argument("--eigen", default="64,128,256", help="sizes of the single-matrix lines ('' for none)")
    ap.add_argument("--batch", default="256x64", help="BATCHxN of the batch line ('' for none)")
    ap.add_argument("--calls", type=int, default=10, help="calls per timed region")
    ap.add_argument("--only", choices=["device", "host", "eigen"],
                    help="only --calls calls of this one on the first configuration (eigen: the first size)")
    ap.add_argument("--eigen-form", type=int, default=0)
    ap.add_argument("--out", help="append the JSON lines to this file too")
    args = ap.parse_args()
    pkg = load_package()
    pkg.set_device(0)
    lib = pkg.lib()

    def ok(rc):
        if rc:
            raise SystemExit(lib.csim_last_error().decode())

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        if args.out:
            with open(args.out, "a") as f:
                f.write(line + "\n")

    sizes = [int(v) for v in args.eigen.split(",") if v]
    if args.only == "eigen":
        A = gram(sizes[0], 1)[None]
        for _ in range(args.calls):
            pkg.sym_eigen_batch(A, form=args.eigen_form)
        return
    single = {}
    for n in sizes if not args.only else []:
        A = gram(n, 1)
        got, want = pkg.sym_eigen_batch(A[None], form=args.eigen_form), pkg.sym_eigen(A, order="round_robin")
        if not (np.array_equal(got.V[0].view(np.int64), want.V.view(np.int64)) and got.sweeps[0] == want.sweeps):
            raise SystemExit(f"n = {n}: the device eigensolver differs from the host order")
        rec = dict(kind="eigen", n=n, form=pkg.sym_eigen_device_form(n, args.eigen_form)[0], sweeps=int(want.sweeps),
                   rotations=int(want.sweeps) * n * (n - 1) // 2, calls=args.calls, regions=REGIONS)
        for name, fn in (("device", lambda: pkg.sym_eigen_batch(A[None], form=args.eigen_form)),
                         ("host_round_robin", lambda: pkg.sym_eigen(A, order="round_robin")),
                         ("host_rows", lambda: pkg.sym_eigen(A))):
            fn()
            med, spread = timed(fn, args.calls if n < 256 or name == "device" else 2)
            rec[name + "_us"], rec[name + "_spread"] = med * 1e6, spread
        single[n] = rec["device_us"]
        emit(rec)
    if args.batch and not args.only:
        batch, n = (int(v) for v in args.batch.split("x"))
        A = np.stack([gram(n, 100 + b) for b in range(batch)])
        fn = lambda: pkg.sym_eigen_batch(A, form=args.eigen_form)  # noqa: E731
        fn()
        med, spread = timed(fn, args.calls)
        one = single.get(n)
        if one is None:
            one = timed(lambda: pkg.sym_eigen_batch(A[:1], form=args.eigen_form), args.calls)[0] * 1e6
        emit(dict(kind="eigen_batch", n=n, batch=batch, batch_us=med * 1e6, batch_spread=spread,
                  matrices_per_s=batch / med, single_us=one, batch_over_singles=med * 1e6 / (batch * one)))

    for cfg in args.config or ["64x512x1024", "64x512x16384", "256x256x1024"]:
        B, n, nobs = (int(v) for v in cfg.split("x"))
        rng = np.random.default_rng(B * 7 + n + nobs)
        X = 1.0 + rng.random((B, n + 2, n + 2))
        e = pkg.Ensemble(B, n, n, 1.0, 1.0, [0, 0, 0, 0])
        e.upload_all(X)
        e.set_option("eigen_form", args.eigen_form)
        cells = rng.permutation(n * n)[:nobs]
        i, j = (cells % n + 1).astype(np.int32), (cells // n + 1).astype(np.int32)
        net = e.obs_network(i, j, rng.uniform(0.5, 2.0, nobs), 4.0)
        net.set_values(1.5 + 0.3 * rng.standard_normal(nobs))

        def sync():
            ok(lib.csim_ensemble_sync(e._h))

        def enqueue():
            ok(lib.csim_ensemble_assimilate_etkf_device(e._h, net._h, 1.0, -1, 0, 0.0))

        def device():
            enqueue()
            sync()

        def host():
            ok(lib.csim_ensemble_assimilate_etkf(e._h, net._h, 1.0, -1, 0, 0.0))
            sync()

        if args.only:
            for _ in range(args.calls):
                {"device": device, "host": host}[args.only]()
            e.close()
            return

        # the two paths agree to rounding on the same members before anything is timed
        device()
        Xd = e.download_all()
        info = e.etkf_info()
        e.upload_all(X)
        host()
        if not np.allclose(Xd, e.download_all(), rtol=0, atol=1e-9):
            raise SystemExit(f"{cfg}: the device analysis differs from the host path")
        e.upload_all(X)
        A = e.obs_gram(net).A
        rec = dict(kind="analysis", config=cfg, members=B, n=n, nobs=nobs, calls=args.calls, regions=REGIONS,
                   eigen_form=pkg.sym_eigen_device_form(B, args.eigen_form)[0], sweeps=info.sweeps)
        slow = B > 128  # the host eigensolver takes 0.2 s there: fewer calls per region
        for name, fn, calls, after in (("obs_gram", lambda: e.obs_gram(net), args.calls, None),
                                       ("etkf_weights", lambda: pkg.etkf_weights(A), 2 if slow else args.calls, None),
                                       ("assimilate_etkf", host, 2 if slow else args.calls, None),
                                       ("device", device, args.calls, None),
                                       ("device_enqueue", enqueue, args.calls, sync)):
            e.upload_all(X)  # every path starts from the same members
            fn()
            sync()
            med, spread = timed(fn, calls, after)
            rec[name + "_us"], rec[name + "_spread"] = med * 1e6, spread
        rec["device_over_host"] = rec["device_us"] / rec["assimilate_etkf_us"]
        e.close()
        emit(rec)


if __name__ == "__main__":
    main()
