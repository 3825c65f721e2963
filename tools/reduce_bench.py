#!/usr/bin/env python3
"""Host-visible cost of the reduction entry points of include/csim.h: microseconds per synchronous call, one JSON
line.  CSIM_LIB picks another build of the engine, so two builds can be alternated (as tools/gpu_lib_ab.sh does).
  csim_stepper_minmax / _sum / _checksum at 16384^2, csim_field_linf_diff at 4096^2,
  csim_ensemble_minmax / _sum / _checksum at 64 x 512^2; --calls per entry point after --warm untimed ones."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from __graft_entry__ import load_package  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--warm", type=int, default=5)
    ap.add_argument("--stepper", type=int, default=16384)
    ap.add_argument("--field", type=int, default=4096)
    ap.add_argument("--ensemble", type=int, nargs=2, default=(64, 512), metavar=("MEMBERS", "N"))
    a = ap.parse_args()
    csim = load_package()
    csim.set_device(0)

    st = csim.Stepper.single(a.stepper, a.stepper)
    st.init_gaussian()
    fa, fb = csim.Field(a.field, a.field), csim.Field(a.field, a.field)
    fa.fill(1.0)
    fb.fill(-2.5)
    B, n = a.ensemble
    e = csim.Ensemble(B, n, n)
    for k in range(B):
        e.init_gaussian(k, A=1.0 + k)
    entries = [("csim_stepper_minmax", st.minmax), ("csim_stepper_sum", st.sum), ("csim_stepper_checksum", st.checksum),
               ("csim_field_linf_diff", lambda: fa.linf_diff(fb)),
               ("csim_ensemble_minmax", lambda: e.minmax().tolist()), ("csim_ensemble_sum", lambda: e.sums().tolist()),
               ("csim_ensemble_checksum", e.checksums)]
    us, values = {}, {}
    for name, call in entries:
        for _ in range(a.warm):
            call()
        t0 = time.perf_counter()
        for _ in range(a.calls):
            r = call()
        us[name] = round((time.perf_counter() - t0) / a.calls * 1e6, 2)
        values[name] = r[-1] if isinstance(r, list) else r  # the last member's result: the same bits from every build
    print(json.dumps({"calls": a.calls, "stepper": a.stepper, "field": a.field, "ensemble": [B, n], "us_per_call": us,
                      "values": values}))
    e.close()
    st.close()


if __name__ == "__main__":
    main()
