#!/usr/bin/env python3
"""What kad_rollout_plan costs at the flagship scale: device time against the bytes it has to move.

    python scripts/rollout_cost.py [--objects 1000000] [--repeat 5]

A synth.gen_rollout batch (mean 8 targets an object) is planned ``repeat`` times after one warm-up; reported are
the median device time of rollout_kernel (kad_rollout_timing), the compulsory bytes (every input read once, every
output written once) and their time at the HBM rate a streaming kernel sustains on an MI355X, the ratio of the
two, and the same call with every group width forced, with long_min lowered so that part of the objects takes the
long path, and with the serial walk forced for every object (kad_rollout_debug_route). One JSON line.
"""
import argparse
import json
import statistics
import sys
import os

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HBM_BYTES_PER_S = 6.3e12  # what a streaming copy achieves of the 8 TB/s peak


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--objects", type=int, default=1_000_000)
    ap.add_argument("--repeat", type=int, default=5)
    args = ap.parse_args()
    from kubeadmiral_amd import build, runtime, synth
    build.build()
    a = synth.gen_rollout(3, args.objects)
    O, T = len(a["obj_flags"]), len(a["tgt_flags"])
    nbytes = 4 * (O + 1) + 13 * O + 41 * T + 14 * T + O  # offsets, object columns, target columns; outputs
    ctx = runtime.Context(0)

    def timed(width=0, long_min=0, serial=0):
        ctx.rollout_debug_route(width, long_min, serial)
        try:
            ctx.rollout_plan(**a)
            ms = []
            for _ in range(args.repeat):
                ctx.rollout_plan(**a)
                ms.append(ctx.rollout_timing()[0])
            return round(statistics.median(ms), 4), ctx.rollout_last_route()
        finally:
            ctx.rollout_debug_route(0, 0, 0)

    ms, route = timed()
    byte_ms = nbytes / HBM_BYTES_PER_S * 1e3
    out = {"objects": O, "targets": T, "route": route, "device_ms": ms, "compulsory_bytes": nbytes,
           "byte_ms": round(byte_ms, 4), "ratio": round(ms / byte_ms, 2),
           "width_sweep_ms": {w: timed(width=w)[0] for w in (1, 2, 4, 8, 16, 32, 64)},
           "long_min_sweep_ms": {lm: timed(long_min=lm)[0] for lm in (8, 12, 14)},
           "serial_ms": timed(serial=1)[0]}
    ctx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
