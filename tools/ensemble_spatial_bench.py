#!/usr/bin/env python3
"""tools/ensemble_spatial_bench.py — cost of the neighbourhood and probability verification
(csim_ensemble_verify_spatial), one JSON line per configuration.

For B members of n x n against a host truth field (M = B forecast members), nt thresholds spread over the data's range:
  quantiles_us  one synchronous csim_ensemble_quantiles with nq = 0, the same thresholds and every output NULL: the
                yardstick of the count pass.  Both read every member once; it writes 8-byte probabilities where the
                count pass writes 2-byte counts.  Its code is the same in this revision and its parent.
  counts_us     one synchronous csim_ensemble_verify_spatial with no scale and every output NULL: the truth's copy, the
                count pass, and a score pass that only histograms (no halo, no window sums).
  scales_us     the same with the half-widths 0, 2, 8, 32; score_over_counts = (scales_us - counts_us) / counts_us and
                hmax_us, one call per largest half-width 0, 2, 8, 32 (one scale each), show what the windows cost.
Every time is the mean over `--calls` calls of one region that ends in a stream synchronise; a configuration takes five
regions after a warm-up and reports their median and spread (max - min).  lds_bytes is the score pass's dynamic LDS
per workgroup at the largest half-width.  The kernels' own durations come from a rocprofv3 --kernel-trace --stats run of
`--only-calls`.  Before timing, the tables are checked against the numpy restatement of tests/spatial_restatement.py at
configurations of up to 2^22 member cells.

  python tools/ensemble_spatial_bench.py --config 64x512 --config 256x256 --config 64x1024 --config 1024x64 [--out F]
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
import spatial_restatement as ref  # noqa: E402

HALVES = [0, 2, 8, 32]
TILE = 32


def regions(fn, calls, n=5):
    out = []
    for _ in range(n):
        t0 = time.perf_counter()
        fn()
        out.append((time.perf_counter() - t0) / calls * 1e6)
    return dict(median=statistics.median(out), spread=max(out) - min(out))


def lds_bytes(M, hmax):
    ww = (TILE + 2 * hmax + 1) ** 2
    r16 = lambda b: (b + 15) // 16 * 16  # noqa: E731
    return 8 * 3 * 8 + 16 + r16(4 * ww) + r16(2 * ww) + 8 * (M + 1)


def default_split(cells, M):
    """ens_spatial_split of csrc/ensemble_spatial.hip: the parts the count pass splits a cell's members into"""
    blocks = (cells + 255) // 256
    if blocks >= 512 or M < 128:
        return 1
    return max(1, min((M + 63) // 64, (1024 + blocks - 1) // blocks))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", action="append", default=[], help="BxN: B members of N x N")
    ap.add_argument("--nt", action="append", type=int, default=[], help="thresholds per call (default 4 and 16)")
    ap.add_argument("--calls", type=int, default=10, help="calls per timed region")
    ap.add_argument("--only-calls", action="store_true", help="only --calls calls of each kind (for a profiler run)")
    ap.add_argument("--out", help="append the JSON lines to this file too")
    args = ap.parse_args()
    pkg = load_package()
    pkg.set_device(0)
    C, lib = pkg.C, pkg.lib()
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int)

    def ck(rc):
        if rc:
            raise SystemExit(lib.csim_last_error().decode())

    for cfg in args.config or ["64x512", "256x256", "64x1024", "1024x64"]:
        B, n = (int(v) for v in cfg.split("x"))
        rng = np.random.default_rng(B * 7 + n)
        e = pkg.Ensemble(B, n, n, 1.0, 1.0, [0, 0, 0, 0])
        x = rng.random((B, n + 2, n + 2))
        e.upload_all(x)
        y = rng.random((n + 2, n + 2))
        yp = y.ctypes.data_as(dp)
        for nt in args.nt or [4, 16]:
            thr = np.linspace(0.1, 0.9, nt)
            tp = thr.ctypes.data_as(dp)
            hs = np.array(HALVES, dtype=np.int32)

            def quant():
                for _ in range(args.calls):
                    ck(lib.csim_ensemble_quantiles(e._h, 0, None, nt, tp, None, None))

            def spatial(ns, h):
                hp = h.ctypes.data_as(ip)

                def go():
                    for _ in range(args.calls):
                        ck(lib.csim_ensemble_verify_spatial(e._h, yp, -1, nt, tp, ns, hp, None, None, None, None, None,
                                                            None))
                return go
            kinds = dict(quantiles_us=quant, counts_us=spatial(0, hs), scales_us=spatial(len(hs), hs))
            ones = [np.array([h], dtype=np.int32) for h in HALVES]
            for h, a in zip(HALVES, ones):
                kinds[f"hmax{h}_us"] = spatial(1, a)
            if args.only_calls:
                for fn in kinds.values():
                    fn()
                continue
            if B * n * n <= 1 << 22 and nt == 4:
                got = e.verify_spatial(y, thresholds=thr, half_widths=HALVES)
                want = ref.restate(x, y, list(thr), HALVES)
                if not (np.array_equal(got.table, want["table"]) and np.array_equal(got.nbh, want["nbh"])):
                    raise SystemExit(f"{cfg}: the tables differ from the numpy restatement")
            rec = dict(config=cfg, members=B, n=n, nt=nt, half_widths=HALVES, calls=args.calls,
                       member_split=default_split(n * n, B), lds_bytes=lds_bytes(B, max(HALVES)),
                       lds_bytes_no_scale=lds_bytes(B, 0), window_sums="summed-area table in LDS",
                       member_bytes=8 * B * n * n)
            for fn in kinds.values():  # warm-up: every kernel and every buffer size once
                fn()
            for k, fn in kinds.items():
                r = regions(fn, args.calls)
                rec[k] = r["median"]
                rec[k.replace("_us", "_spread_us")] = r["spread"]
            rec["counts_over_quantiles"] = rec["counts_us"] / rec["quantiles_us"]
            rec["counts_within_yardstick"] = rec["counts_us"] <= rec["quantiles_us"] + 2 * rec["quantiles_spread_us"]
            rec["score_over_counts"] = (rec["scales_us"] - rec["counts_us"]) / rec["counts_us"]
            rec["counts_gbps"] = rec["member_bytes"] / rec["counts_us"] / 1e3
            line = json.dumps(rec)
            print(line, flush=True)
            if args.out:
                with open(args.out, "a") as f:
                    f.write(line + "\n")
        e.close()


if __name__ == "__main__":
    main()
