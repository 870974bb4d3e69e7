#!/usr/bin/env python3
"""What kad_revision_plan costs, per kernel, per lane-group width and per path.

    python scripts/history_cost.py [--objects 1000,10000,100000] [--repeat 5] [--out FILE]

Batches of synth.gen_revisions (history 2: three strings of about 1.8 KB an object). For each size: the medians of
kad_revision_plan_timing's three intervals (hr_hash_kernel, hr_compare_kernel, hr_plan_kernel) and of the call's wall
time after a warm-up, on the route's own choice, at lane-group widths forced through kad_revision_plan_debug_route and
with every object with revisions on the long path; next to history.plan_numpy on the same arrays and tests/history_ref.py on
the same objects (every ``--ref-every``-th object where that is above 1: the figure is then scaled and says so). The
compare kernel's bytes are the data and the patch of every pair whose lengths agree (the synthetic old revisions
differ in one byte behind the env list, so nearly all of both is read), against an HBM peak of 8 TB/s. One JSON line per
measurement."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
HBM_PEAK_GBPS = 8000.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--objects", default="1000,10000,100000")
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--ref-every", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import numpy as np

    import history_ref
    from kubeadmiral_amd import build, history, runtime, synth
    build.build()
    ctx = runtime.Context(0)
    sink = open(args.out, "w") if args.out else None

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        if sink:
            sink.write(line + "\n")
            sink.flush()

    sizes = [int(x) for x in args.objects.split(",")]
    for O in sizes:
        t0 = time.perf_counter()
        batch = synth.gen_revisions(5, O, history=2)
        a = batch.arrays()
        pack_ms = round((time.perf_counter() - t0) * 1e3, 1)
        t0 = time.perf_counter()
        want = history.plan_numpy(**a)
        numpy_ms = round((time.perf_counter() - t0) * 1e3, 1)
        every = args.ref_every if O > 20000 else 1
        t0 = time.perf_counter()
        ref = [history_ref.sync_revisions(e) for e in batch.objs[::every]]
        ref_ms = round((time.perf_counter() - t0) * 1e3 * every, 1)
        same_len = a["rev_data_len"] == np.repeat(a["patch_len"], np.diff(a["rev_off"]))
        cmp_bytes = int(2 * a["rev_data_len"][same_len].astype(np.int64).sum())
        shape = {"objects": O, "revisions": int(len(a["rev_flags"])), "blob_mb": round(len(a["blob"]) / 1e6, 1), "pack_ms": pack_ms,
                 "numpy_ms": numpy_ms, "ref_ms": ref_ms, "ref_every": every, "cmp_bytes": cmp_bytes}
        variants = [("own", 0, 0)] + [(f"w{w}", w, 1 << 30) for w in ((1, 2, 4, 8, 16, 32, 64) if O <= 20000 else (1, 4, 16, 64))] + [("block", 0, 1)]
        for label, width, long_min in variants:
            ctx.revision_plan_debug_route(width, long_min)
            got = {}
            call = lambda: got.update(ctx.revision_plan(**a))  # noqa: E731
            call()
            ms, wall = [], []
            for _ in range(args.repeat):
                t0 = time.perf_counter()
                call()
                wall.append((time.perf_counter() - t0) * 1e3)
                ms.append(ctx.revision_plan_timing())
            k = [round(statistics.median(m[i] for m in ms), 4) for i in range(3)]
            same = all(np.array_equal(got[f], want[f]) for f in ("hash", "equal", "n_old", "keep", "n_actions", "last", "rev_number"))
            if label == "own":
                same = same and [history_ref.outcome_tuple(o) for o in batch.apply(got)[::every]] == ref
            emit({**shape, "variant": label, "route": ctx.revision_plan_last_route(), "hash_ms": k[0], "cmp_ms": k[1], "plan_ms": k[2],
                  "wall_ms": round(statistics.median(wall), 3), "cmp_gbps": round(cmp_bytes / max(k[1], 1e-6) / 1e6, 1),
                  "cmp_of_peak": round(cmp_bytes / max(k[1], 1e-6) / 1e6 / HBM_PEAK_GBPS, 4), "equal": bool(same)})
        ctx.revision_plan_debug_route(0, 0)
    ctx.close()


if __name__ == "__main__":
    main()
