#!/usr/bin/env python3
"""What kad_deletion_plan and kad_deletion_finish cost at the flagship scale: each kernel against the bytes it has to
move, and against the copies either side of it.

    python scripts/deletion_cost.py [--objects 1000000] [--clusters 1000] [--repeat 5] [--sample 2000] [--widths]

A synth.gen_deletion batch (about 10 observed clusters an object, one object in five observed nowhere) goes through both
calls ``repeat`` times after one warm-up; reported per call are the medians of its timing's three intervals (inputs to
the device, deletion_count_kernel + deletion_kernel, outputs back), the wall time of the whole call, the compulsory
bytes of the kernels (every input read once, every output written once) with the rate achieved on them and their time
at the HBM rate a streaming kernel sustains on an MI355X, the numpy restatement's time on the same batch, and the
per-object reference's time on a sample (tests/deletion_ref.py), scaled to the batch. ``--widths`` adds the kernels'
medians at every forced lane-group width. One JSON line.
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
    ap.add_argument("--widths", action="store_true")
    args = ap.parse_args()
    import numpy as np

    import deletion_cases as DC
    import deletion_ref
    from kubeadmiral_amd import build, deletion, runtime, synth
    build.build()
    a = synth.gen_deletion(3, args.objects, args.clusters)
    plan_a = {k: a[k] for k in synth.DELETION_PLAN_KEYS}
    O, B, K, C = len(a["obj_flags"]), len(a["ob_cluster"]), len(a["chk_cluster"]), args.clusters
    ctx = runtime.Context(0)
    calls = {"plan": (lambda: ctx.deletion_plan(**plan_a), ctx.deletion_timing, ctx.deletion_last_route, ctx.deletion_debug_route),
             "finish": (lambda: ctx.deletion_finish(**a), ctx.deletion_finish_timing, ctx.deletion_finish_last_route,
                        ctx.deletion_finish_debug_route)}
    # every input read once, every output written once (the cluster bytes once a launch, not once a block)
    nbytes = {"plan": C + O + 4 * (O + 1) + 5 * B + B + 14 * O,
              "finish": 2 * C + O + 4 * (O + 1) + 5 * B + B + O + 4 * (O + 1) + 5 * K + 11 * O}
    med = lambda v: round(statistics.median(v), 4)  # noqa: E731
    out = {"objects": O, "clusters": C, "observations": B, "check_rows": K}
    got = {}
    for name, (call, timing, last_route, debug_route) in calls.items():
        got[name] = call()
        h2d, kernel, d2h, wall = [], [], [], []
        for _ in range(args.repeat):
            t0 = time.perf_counter()
            call()
            wall.append((time.perf_counter() - t0) * 1e3)
            ms = timing()
            h2d.append(ms[0])
            kernel.append(ms[1])
            d2h.append(ms[2])
        byte_ms = nbytes[name] / HBM_BYTES_PER_S * 1e3
        out[name] = {"route": last_route(), "h2d_ms": med(h2d), "kernel_ms": med(kernel), "d2h_ms": med(d2h), "call_wall_ms": med(wall),
                     "compulsory_bytes": nbytes[name], "kernel_bytes_per_s": round(nbytes[name] / (med(kernel) * 1e-3)),
                     "byte_ms": round(byte_ms, 4), "ratio": round(med(kernel) / byte_ms, 2)}
        if args.widths:
            by_width = {}
            for w in (1, 2, 4, 8, 16, 32, 64):
                debug_route(w, 0)
                call()
                ks = []
                for _ in range(args.repeat):
                    call()
                    ks.append(timing()[1])
                by_width[w] = med(ks)
            debug_route(0, 0)
            out[name]["kernel_ms_by_width"] = by_width
    ctx.close()
    t0 = time.perf_counter()
    want = deletion.plan_numpy(**plan_a)
    out["plan"]["numpy_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
    t0 = time.perf_counter()
    want_fin = deletion.finish_numpy(**a)
    out["finish"]["numpy_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
    assert all((np.asarray(want[k]) == got["plan"][k]).all() for k in want)
    assert all((np.asarray(want_fin[k]) == got["finish"][k]).all() for k in want_fin)
    # the per-object reference on the first objects, scaled
    n = min(args.sample, O)
    names = DC.cluster_names(C)
    worlds = DC.worlds_of_arrays(a, range(n))
    cl = list(zip(names, (a["cluster_flags"] & 1).astype(bool).tolist()))
    cl2 = list(zip(names, (a["chk_cluster_flags"] & 1).astype(bool).tolist()))
    t0 = time.perf_counter()
    for w in worlds:
        deletion_ref.reconcile(w, cl, cl2)
    out["ref_ms_scaled"] = round((time.perf_counter() - t0) * 1e3 * O / n, 1)
    out["ref_sample"] = n
    print(json.dumps(out))


if __name__ == "__main__":
    main()
