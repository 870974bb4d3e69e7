#!/usr/bin/env python3
"""Device time of one kad_migrate_estimate on the scale of the c3 bench workload.

    python scripts/migrate_cost.py [--config c3] [--objects N] [--runs 10] [--warmup 2] [--alternatives]

synth.gen_migration makes one object per unit of the config (1M at c3), each on 1-5 member clusters, a segment
holding about as many pods as the synthetic Deployments have replicas (1-100). Two workloads: steady state
(90 % of the segments have total == ready and carry no pods) and cold (every segment carries pods).
kad_migrate_timing's HIP events give the segment and the object kernel per call (medians of ``runs``). Beside
them stand: the host-to-device time of the same arrays as its own figure (pageable host memory, through torch);
the bytes that must move — pod columns (8 + 1 B a pod of a counted segment), segment columns (cluster 4,
desired 8, flags 1, pod offset 8, object index 4 B) and object columns (segment offset 4, threshold 8, old
offset 4 B, 12 B an old entry), outputs (20 B a segment, 14 B an object) — and their time at the HBM rate
measured as achievable on an MI355X (6.3 TB/s); the ratio of kernel time to that byte time; and, for
comparison only, automigration.migrate_numpy, a single-thread numpy restatement (np.add.reduceat) on the same
arrays. ``--alternatives``: the cold workload again under other group widths and long_min values
(kad_migrate_debug_route), with a tenth of the objects holding one segment of 2000-6000 pods for long_min.
Prints one JSON line."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_ACHIEVABLE = 6.3e12  # B/s
IN_KEYS = ("obj_seg_off", "obj_threshold_ns", "seg_cluster", "seg_desired", "seg_flags", "seg_pod_off", "pod_t_ns",
           "pod_flags", "old_off", "old_cluster", "old_cap")


def byte_model(a):
    O, S = len(a["obj_threshold_ns"]), len(a["seg_cluster"])
    live = (a["seg_flags"] & 1) == 0
    pods = int(np.diff(a["seg_pod_off"])[live].sum())
    seg_in = {"pod_columns": 9 * pods, "segment_columns": S * (4 + 8 + 1 + 8 + 4), "outputs": 20 * S}
    obj_in = {"segment_columns": S * (1 + 8 + 8 + 4), "object_columns": O * (4 + 8 + 4) + 12 * len(a["old_cluster"]),
              "outputs": 14 * O}
    return seg_in, obj_in


def h2d_ms(a, runs):
    import torch
    ts = []
    for _ in range(runs):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        keep = [torch.from_numpy(a[k]).cuda() for k in IN_KEYS if len(a[k])]
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
        del keep
    return float(np.median(ts))


def measure(ctx, a, runs, warmup):
    times = []
    for i in range(warmup + runs):
        r = ctx.migrate_estimate(**a)
        if i >= warmup:
            times.append(ctx.migrate_timing())
    return np.median(np.array(times), axis=0), r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="c3")
    ap.add_argument("--objects", type=int, default=0)
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--alternatives", action="store_true")
    a = ap.parse_args()
    import torch  # noqa: F401

    import bench
    from kubeadmiral_amd import automigration as AM
    from kubeadmiral_amd import runtime, synth
    from kubeadmiral_amd.pack import Snapshot

    W0, C = synth.SIZES[a.config]
    W = a.objects or W0
    ctx = runtime.Context(0)
    ctx.upload_snapshot(Snapshot(bench.make_clusters(a.config, C)))
    out = {"config": a.config, "objects": W, "clusters": C, "counter_run": False}
    for name, share in (("steady", 0.9), ("cold", 0.0)):
        arr, stale = synth.gen_migration(0, W, C, ready_share=share, changed=0.05)
        t, r = measure(ctx, arr, a.runs, a.warmup)
        seg_b, obj_b = byte_model(arr)
        floor = [sum(seg_b.values()) / HBM_ACHIEVABLE * 1e3, sum(obj_b.values()) / HBM_ACHIEVABLE * 1e3]
        t0 = time.perf_counter()
        ref = AM.migrate_numpy(**arr)
        numpy_ms = (time.perf_counter() - t0) * 1e3
        out[name] = {"segments": len(arr["seg_cluster"]), "pods": len(arr["pod_t_ns"]), "changed": int(r["changed"].sum()),
                     "segment_ms": round(float(t[0]), 4), "object_ms": round(float(t[1]), 4),
                     "h2d_ms_pageable_torch": round(h2d_ms(arr, 3), 3),
                     "segment_bytes": seg_b, "object_bytes": obj_b,
                     "segment_ms_at_hbm": round(floor[0], 4), "object_ms_at_hbm": round(floor[1], 4),
                     "segment_ratio": round(float(t[0]) / floor[0], 1), "object_ratio": round(float(t[1]) / floor[1], 1),
                     "numpy_single_thread_ms": round(numpy_ms, 1),
                     "equals_numpy": all((r[k] == ref[k]).all() for k in ref), "route": ctx.migrate_last_route()}
        if name == "cold" and a.alternatives:
            alt = {}
            for w in (8, 16, 32, 64):
                ctx.migrate_debug_route(w, 0)
                t, r2 = measure(ctx, arr, a.runs, a.warmup)
                alt[f"width_{w}"] = {"segment_ms": round(float(t[0]), 4), "equal": all((r2[k] == ref[k]).all() for k in ref)}
            ctx.migrate_debug_route(0, 0)
            # long segments for long_min: every tenth object gets one segment of 2000-6000 pods
            big, _ = synth.gen_migration(1, W // 10, C, ready_share=0.0, max_segments=1, replicas=(2000, 6000), changed=0.0)
            refb = AM.migrate_numpy(**big)
            for lm in (256, 1024, 4096, 1 << 30):
                ctx.migrate_debug_route(0, lm)
                t, r2 = measure(ctx, big, a.runs, a.warmup)
                alt[f"long_min_{lm}"] = {"segment_ms": round(float(t[0]), 4), "long_grid": ctx.migrate_last_route()["long_grid"],
                                         "pods": len(big["pod_t_ns"]), "equal": all((r2[k] == refb[k]).all() for k in refb)}
            ctx.migrate_debug_route(0, 0)
            out["alternatives"] = alt
    print(json.dumps(out))


if __name__ == "__main__":
    main()
