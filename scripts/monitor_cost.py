#!/usr/bin/env python3
"""What the monitor's two calls cost on a resident table: kad_monitor_report against the 45 B a slot it must read,
on both histogram paths, and against the numpy restatement on the same table; kad_monitor_reconcile for a batch of
events against a table of that size.

    python scripts/monitor_cost.py [--slots 1000000,10000000] [--repeat 5] [--events 100000] [--clusters 8]

For every table size the table is filled through kad_monitor_load with a seeded mix (a share ``--late`` of the meters
not synced, a share ``--fresh`` synced within the interval, the rest synced long ago; eight kinds), then the report
runs ``repeat`` times after a warm-up on the route's own path and with each path forced
(kad_monitor_report_debug_route), once more with 4096 types. One JSON line a row: the medians of
kad_monitor_report_timing's intervals (the zeroing, monitor_scan_kernel, the offsets and monitor_scatter_kernel), the
scan's effective bytes per second over n_slots * 45 B, the share of what a streaming kernel sustains on an MI355X,
the timers it emitted, and report_numpy's wall time on the mirror. Then one reconcile of ``events`` synced objects
with ``clusters`` entries a list: kad_monitor_reconcile_timing's intervals and reconcile_numpy's wall time.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_BYTES_PER_S = 6.3e12  # what a streaming copy achieves of the 8 TB/s peak
SLOT_BYTES = 45


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--slots", default="1000000,10000000")
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--events", type=int, default=100_000)
    ap.add_argument("--clusters", type=int, default=8)
    ap.add_argument("--late", type=float, default=0.02)
    ap.add_argument("--fresh", type=float, default=0.05)
    args = ap.parse_args()
    import numpy as np

    from kubeadmiral_amd import build, monitor as M, runtime
    build.build()
    ctx = runtime.Context(0)
    med = lambda v: round(statistics.median(v), 4)  # noqa: E731
    now, S = 1_700_000_000 * 10 ** 9, 10 ** 9
    for n in (int(x) for x in args.slots.split(",")):
        rng = np.random.default_rng(n)
        mir = M.Mirror()
        mir.ensure(n)
        mir.n_slots = n
        cr = now - rng.integers(3600, 30 * 86400, n) * S
        r = rng.random(n)
        ss = np.where(r < args.late, cr - S, np.where(r < args.late + args.fresh, now - rng.integers(0, 60, n) * S,
                                                     cr + rng.integers(1, 600, n) * S))
        lu = np.where(rng.random(n) < 0.5, M.TIME_ZERO, cr + S)
        lu = np.where(r < args.late, now - rng.integers(0, 2 * 86400, n) * S, np.minimum(lu, ss - S))
        mir.cols[:] = (cr, lu, ss, now - rng.integers(0, 600, n) * S, np.zeros(n, np.int64))
        mir.type_id[:n] = rng.integers(0, 8, n)
        mir.flags[:n] = rng.random(n) < 0.97
        ctx.monitor_clear()
        ctx.monitor_reserve(n)
        ctx.monitor_load(np.arange(n, dtype=np.int32), type_id=mir.type_id[:n], flags=mir.flags[:n],
                         **{k: mir.cols[i, :n] for i, k in enumerate(M.COLUMNS)})
        for n_types, forces in ((8, (0, 1, 2)), (4096, (1, 2))):
            t0 = time.perf_counter()
            want = M.report_numpy(mir, now, n_types)
            numpy_ms = (time.perf_counter() - t0) * 1e3
            for force in forces:
                ctx.monitor_report_debug_route(force, 0)
                ms = []
                for k in range(args.repeat + 1):
                    got = ctx.monitor_report(now, n_types, timer_cap=int(want["n_timers"].max()) + 1)
                    if k:
                        ms.append(ctx.monitor_report_timing())
                for key in ("counters", "type_sync", "type_status", "sync_slot", "sync_ms", "status_slot", "status_ms"):
                    assert got[key].tobytes() == want[key].tobytes(), key
                scan = med([m[1] for m in ms])
                route = ctx.monitor_report_last_route()
                rate = n * SLOT_BYTES / (scan * 1e-3)
                print(json.dumps({"call": "report", "n_slots": n, "n_types": n_types, "forced": force,
                                  "path": runtime.MONITOR_PATHS[route["path"]], "grid": route["grid"],
                                  "zero_ms": med([m[0] for m in ms]), "scan_ms": scan,
                                  "timers_ms": med([m[2] for m in ms]), "scan_bytes_per_s": round(rate / 1e12, 3),
                                  "scan_share_of_stream": round(rate / HBM_BYTES_PER_S, 3),
                                  "timers": [int(x) for x in got["n_timers"]], "numpy_ms": round(numpy_ms, 2)}), flush=True)
            ctx.monitor_report_debug_route(0, 0)
        # one batch of synced events over existing slots
        E, C = min(args.events, n), args.clusters
        slots = rng.choice(n, E, replace=False).astype(np.int32)
        slots = slots[mir.flags[slots] == 1]
        E = len(slots)
        off = (np.arange(E + 1) * C).astype(np.int32)
        cl = np.tile(np.arange(C, dtype=np.int32), E)
        gen = np.ones(E * C, np.int64)
        a = dict(n_clusters=C, now_ns=now, slot=slots, type_id=mir.type_id[slots],
                 obj_flags=np.full(E, M.SS_PARSED | M.LASTGEN_PRESENT | M.LASTGEN_EQUAL | M.STATUS_ENABLED | M.HAS_LAST, np.uint16),
                 creation_ns=np.zeros(E, np.int64), sync_success_ns=np.full(E, now - S, np.int64))
        for name in ("fed", "mem", "last"):
            a.update({name + "_off": off, name + "_cluster": cl, name + "_gen": gen})
        ms = []
        for k in range(args.repeat + 1):
            got = ctx.monitor_reconcile(**a)
            if k:
                ms.append(ctx.monitor_reconcile_timing())
        t0 = time.perf_counter()
        want = M.reconcile_numpy(mir, **a)
        numpy_ms = (time.perf_counter() - t0) * 1e3
        for key in ("result", "bits", "meter", "would"):
            assert got[key].tobytes() == want[key].tobytes(), key
        route = ctx.monitor_reconcile_last_route()
        print(json.dumps({"call": "reconcile", "n_slots": n, "events": E, "clusters": C, "width": route["width"],
                          "grid": route["grid"], "in_ms": med([m[0] for m in ms]), "kernel_ms": med([m[1] for m in ms]),
                          "out_ms": med([m[2] for m in ms]), "numpy_ms": round(numpy_ms, 2)}), flush=True)


if __name__ == "__main__":
    main()
