#!/usr/bin/env python3
"""What kad_dispatch_plan costs at the flagship scale: the kernel against the bytes it has to move, and against the
copies either side of it.

    python scripts/dispatch_cost.py [--objects 1000000] [--clusters 1000] [--repeat 5] [--sample 2000]

A synth.gen_dispatch batch (about 5 placed and 5 observed clusters an object) is planned ``repeat`` times after one
warm-up; reported are the medians of kad_dispatch_timing's three intervals (inputs to the device, dispatch_wave_kernel,
outputs back), the wall time of the whole call, the compulsory bytes of the kernel (every input read once, every
emitted entry and per-object column written once) with the rate the kernel achieves on them and their time at the HBM
rate a streaming kernel sustains on an MI355X, the numpy restatement's time on the same batch, and the per-object
checker's time on a sample (tests/dispatch_ref.py), scaled to the batch. One JSON line.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

HBM_BYTES_PER_S = 6.3e12  # what a streaming copy achieves of the 8 TB/s peak


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--objects", type=int, default=1_000_000)
    ap.add_argument("--clusters", type=int, default=1000)
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--sample", type=int, default=2000)
    args = ap.parse_args()
    import numpy as np

    import dispatch_ref
    from kubeadmiral_amd import build, dispatch, runtime, synth
    build.build()
    a = synth.gen_dispatch(3, args.objects, args.clusters)
    O, P, B = len(a["obj_flags"]), len(a["pl_cluster"]), len(a["ob_cluster"])
    ctx = runtime.Context(0)
    got = ctx.dispatch_plan(**a)
    E = int(got["count"].sum())
    in_bytes = sum(np.asarray(v).nbytes for v in a.values())
    h2d, kernel, d2h, wall = [], [], [], []
    for _ in range(args.repeat):
        t0 = time.perf_counter()
        ctx.dispatch_plan(**a)
        wall.append((time.perf_counter() - t0) * 1e3)
        ms = ctx.dispatch_timing()
        h2d.append(ms[0])
        kernel.append(ms[1])
        d2h.append(ms[2])
    route = ctx.dispatch_last_route()
    ctx.close()
    med = lambda v: round(statistics.median(v), 4)  # noqa: E731
    nbytes = in_bytes + 6 * E + 13 * O
    t0 = time.perf_counter()
    ref = dispatch.plan_numpy(**a)
    numpy_ms = (time.perf_counter() - t0) * 1e3
    assert all((np.asarray(ref[k]) == got[k]).all() for k in ("count", "n_ops", "n_selected", "obj_result"))
    n = min(args.sample, O)
    head = dict(a, obj_flags=a["obj_flags"][:n], obj_ns=a["obj_ns"][:n], obj_pl_off=a["obj_pl_off"][:n + 1],
                obj_ob_off=a["obj_ob_off"][:n + 1], out_off=a["out_off"][:n + 1])
    t0 = time.perf_counter()
    dispatch_ref.run(**head)
    checker_ms = (time.perf_counter() - t0) * 1e3 * O / n
    out = {"objects": O, "clusters": args.clusters, "placement_entries": P, "observations": B, "entries": E, "route": route,
           "h2d_ms": med(h2d), "kernel_ms": med(kernel), "d2h_ms": med(d2h), "call_wall_ms": med(wall),
           "input_bytes": in_bytes, "compulsory_bytes": nbytes, "kernel_bytes_per_s": round(nbytes / (med(kernel) * 1e-3)),
           "byte_ms": round(nbytes / HBM_BYTES_PER_S * 1e3, 4), "ratio": round(med(kernel) / (nbytes / HBM_BYTES_PER_S * 1e3), 2),
           "plan_numpy_ms": round(numpy_ms, 1), "checker_ms_scaled": round(checker_ms, 1), "checker_sample": n}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
