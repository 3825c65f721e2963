#!/usr/bin/env python3
"""tools/ensemble_held_bench.py — cost of the 4D-ETKF's pieces (csim_obs_network_hold, csim_ensemble_obs_gram_held,
csim_ensemble_assimilate_etkf_held), one JSON line per configuration.  The method of tools/ensemble_etkf_bench.py: ten
calls per timed region, five regions, the median and the spread (max - min) / median reported.

For B members of n x n (all of them forecast members) and a network of nobs point observations at distinct random cells,
spread evenly over 16 time slots:
  hold_slot_us        csim_obs_network_hold of one slot of the 16, then a sync (one wave per observation of the slot);
  hold_all_us         the same with slot = -1, every observation;
  obs_gram_held_us    csim_ensemble_obs_gram_held, A only (two kernels, the copy of A and one stream sync);
  obs_gram_us         csim_ensemble_obs_gram on the same network and the same members: the gathering one;
  etkf_held_us, etkf_held_device_us   hold(-1), csim_ensemble_assimilate_etkf_held on the host / device path, then a
                      sync: a held analysis ends its window, so every call needs its hold, which hold_all_us prices;
  etkf_us, etkf_device_us             csim_ensemble_assimilate_etkf / _etkf_device, then a sync.
Ratios: obs_gram_held_over_obs_gram, etkf_held_over_etkf, etkf_held_device_over_etkf_device.  Before timing, the held
matrix is checked against the gathering one bit for bit (the rows are held from the members it gathers from).

  python tools/ensemble_held_bench.py --config 64x512x1024 --config 64x512x16384 [--out FILE]
"""
import argparse
import ctypes
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
SLOTS = 16


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
    ap.add_argument("--only", choices=["hold_slot", "obs_gram_held", "etkf_held_device"],
                    help="only --calls calls of this one (for a profiler or counter run)")
    ap.add_argument("--obs-gram-form", type=int, default=0)
    ap.add_argument("--out", help="append the JSON lines to this file too")
    args = ap.parse_args()
    pkg = load_package()
    pkg.set_device(0)
    lib = pkg.lib()

    def ok(rc):
        if rc:
            raise SystemExit(lib.csim_last_error().decode())

    for cfg in args.config or ["64x512x1024", "64x512x16384"]:
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
        net = e.obs_network(i, j, r, 4.0)
        net.set_values(y)
        net.set_slots(np.arange(nobs) % SLOTS)

        def hold_slot():
            ok(lib.csim_obs_network_hold(net._h, 5, -1))
            ok(lib.csim_ensemble_sync(e._h))

        def hold_all():
            ok(lib.csim_obs_network_hold(net._h, -1, -1))
            ok(lib.csim_ensemble_sync(e._h))

        Ah, Ag = np.empty((B + 1, B + 1)), np.empty((B + 1, B + 1))
        dptr = ctypes.POINTER(ctypes.c_double)

        def obs_gram_held():  # both through the C entry points, into arrays made once
            ok(lib.csim_ensemble_obs_gram_held(e._h, net._h, Ah.ctypes.data_as(dptr), None, None))
            return Ah

        def obs_gram():
            ok(lib.csim_ensemble_obs_gram(e._h, net._h, -1, Ag.ctypes.data_as(dptr), None, None))
            return Ag

        def analysis(held, device):
            def run():
                if held:
                    ok(lib.csim_obs_network_hold(net._h, -1, -1))
                    ok(lib.csim_ensemble_assimilate_etkf_held(e._h, net._h, 1.0, -1, 0, 0.0, device))
                elif device:
                    ok(lib.csim_ensemble_assimilate_etkf_device(e._h, net._h, 1.0, -1, 0, 0.0))
                else:
                    ok(lib.csim_ensemble_assimilate_etkf(e._h, net._h, 1.0, -1, 0, 0.0))
                ok(lib.csim_ensemble_sync(e._h))
            return run

        hold_all()
        if args.only:
            fn = {"hold_slot": hold_slot, "obs_gram_held": obs_gram_held, "etkf_held_device": analysis(True, 1)}[args.only]
            for _ in range(args.calls):
                fn()
            e.close()
            continue

        A, want = obs_gram_held(), obs_gram()
        if not np.array_equal(A.view(np.int64), want.view(np.int64)):
            raise SystemExit(f"{cfg}: the Gram matrix from held rows differs from the gathering one")

        rec = dict(config=cfg, members=B, n=n, nobs=nobs, slots=SLOTS, slot_obs=int(np.count_nonzero(np.arange(nobs) % SLOTS == 5)),
                   calls=args.calls, regions=REGIONS, obs_gram_form=args.obs_gram_form)
        for name, fn in (("hold_slot", hold_slot), ("hold_all", hold_all), ("obs_gram_held", obs_gram_held),
                         ("obs_gram", obs_gram), ("etkf_held", analysis(True, 0)), ("etkf", analysis(False, 0)),
                         ("etkf_held_device", analysis(True, 1)), ("etkf_device", analysis(False, 1))):
            if name.startswith("etkf"):
                e.upload_all(X)  # every analysis starts from the same members
            fn()
            med, spread = timed(fn, args.calls)
            rec[name + "_us"], rec[name + "_spread"] = med * 1e6, spread
        rec["obs_gram_held_over_obs_gram"] = rec["obs_gram_held_us"] / rec["obs_gram_us"]
        rec["etkf_held_over_etkf"] = rec["etkf_held_us"] / rec["etkf_us"]
        rec["etkf_held_device_over_etkf_device"] = rec["etkf_held_device_us"] / rec["etkf_device_us"]
        e.close()
        line = json.dumps(rec)
        print(line, flush=True)
        if args.out:
            with open(args.out, "a") as f:
                f.write(line + "\n")


if __name__ == "__main__":
    main()
