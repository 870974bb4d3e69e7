#!/usr/bin/env python3
"""What kad_sync_finish and kad_sync_needs_update cost, per lane-group width and per path.

    python scripts/syncfin_cost.py [--objects 100000] [--repeat 5] [--out FILE]

Batches of synth.gen_sync_finish: ``objects`` objects x {8, 64, 1024} touched clusters, and 64 objects x 16384
clusters. For each: the medians of kad_sync_finish_timing's three intervals (inputs to the device, syncfin_kernel,
outputs back) at every lane-group width forced through kad_sync_finish_debug_route, on the block path (long_min
forced below the object size) and on the route's own choice, next to syncfin.finish_numpy on the same arrays; then
kad_sync_needs_update on one row per record with its three intervals and needs_update_numpy. One JSON line per
measurement."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HEAD = ("n_clusters", "n_reasons", "reason_check_clusters", "reason_ns_not_federated")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--objects", type=int, default=100_000)
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import numpy as np

    from kubeadmiral_amd import build, runtime, synth, syncfin
    build.build()
    ctx = runtime.Context(0)
    sink = open(args.out, "w") if args.out else None

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        if sink:
            sink.write(line + "\n")
            sink.flush()

    def timed(call, timing):
        call()
        ms, wall = [], []
        for _ in range(args.repeat):
            t0 = time.perf_counter()
            call()
            wall.append((time.perf_counter() - t0) * 1e3)
            ms.append(timing())
        return [round(statistics.median(m[i] for m in ms), 4) for i in range(3)], round(statistics.median(wall), 3)

    for W, C, touched in ((args.objects, 1024, 8), (args.objects, 1024, 64), (args.objects, 1024, 1024), (64, 16384, 16384)):
        a = synth.gen_sync_finish(5, W, C, touched)
        head = [a[k] for k in HEAD]
        rest = {k: v for k, v in a.items() if k not in HEAD}
        t0 = time.perf_counter()
        want = syncfin.finish_numpy(**a)
        numpy_ms = round((time.perf_counter() - t0) * 1e3, 2)
        shape = {"objects": W, "clusters": C, "touched": touched}
        for label, width, long_min in [("own", 0, 0)] + [(f"w{w}", w, 1 << 30) for w in (1, 2, 4, 8, 16, 32, 64)] + \
                [("block", 0, max(1, touched - 1))]:
            ctx.sync_finish_debug_route(width, long_min)
            got = {}
            (t_in, t_k, t_out), wall = timed(lambda: got.update(ctx.sync_finish(*head, **rest)), ctx.sync_finish_timing)
            same = all(np.array_equal(got[k], want[k]) for k in ("ver_count", "ver_write", "st_count", "obj_out", "reason_out"))
            emit({"call": "finish", **shape, "variant": label, "route": ctx.sync_finish_last_route(), "in_ms": t_in,
                  "kernel_ms": t_k, "out_ms": t_out, "wall_ms": wall, "numpy_ms": numpy_ms, "equal": bool(same)})
        ctx.sync_finish_debug_route(0, 0)
        # the version check: one row per record, the recorded versions = the stored ones
        n = len(a["ent_cluster"])
        rows = {"row_obj": np.repeat(np.arange(W, dtype=np.int32), np.diff(a["ent_off"])), "row_cluster": a["ent_cluster"],
                "row_target": np.maximum(a["ent_version"], 1), "row_flags": np.full(n, 15, np.uint8),
                "obj_flags": np.ones(W, np.uint8), "rec_off": a["oldv_off"], "rec_cluster": a["oldv_cluster"],
                "rec_version": a["oldv_version"], "ver_flags": a["ver_flags"]}
        t0 = time.perf_counter()
        want = syncfin.needs_update_numpy(C, **rows)
        numpy_ms = round((time.perf_counter() - t0) * 1e3, 2)
        got = {}
        (t_in, t_k, t_out), wall = timed(lambda: got.update(ctx.sync_needs_update(C, **rows)), ctx.sync_needs_update_timing)
        emit({"call": "needs_update", **shape, "rows": n, "route": ctx.sync_needs_update_last_route(), "in_ms": t_in,
              "kernel_ms": t_k, "out_ms": t_out, "wall_ms": wall, "numpy_ms": numpy_ms,
              "equal": bool(all(np.array_equal(got[k], want[k]) for k in want))})
    ctx.close()


if __name__ == "__main__":
    main()
