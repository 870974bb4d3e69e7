#!/usr/bin/env python3
"""Device time of one kad_cluster_resources on the scale of a live federation.

    python scripts/cstat_cost.py [--clusters 1000] [--nodes-median 300] [--runs 10] [--warmup 2] [--alternatives]

synth.gen_cluster_status makes the nodes and pods of ``--clusters`` member clusters with skewed sizes (at the
defaults about 1e6 nodes and several 1e7 pods). kad_cstat_timing's HIP events give the node pass and the pod pass
(with its combine kernel) per call (medians of ``runs``). Beside them stand: the host-to-device time of the same
arrays as its own figure (pageable host memory, through torch); the bytes that must move — entry columns (9 B a
node entry, 10 B a pod entry), offsets (8 B a node, a pod and twice a cluster), flags (1 B a node and a pod) and
outputs (16 B a cluster and resource, 16 B a cluster; the pod pass reads alloc and has back) — and their time
at the HBM rate measured as achievable on an MI355X (6.3 TB/s); the ratio of kernel time to that byte time; and,
for comparison only, clusterstatus.cstat_numpy, a single-thread numpy restatement on the same arrays.
``--alternatives``: the same workload under the group widths 8 / 16 / 32 / 64 and other long_min values
(kad_cstat_debug_route). Prints one JSON line."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_ACHIEVABLE = 6.3e12  # B/s
IN_KEYS = ("cl_node_off", "node_flags", "node_ent_off", "nent_res", "nent_val", "cl_pod_off", "pod_flags", "pod_ent_off",
           "pent_res", "pent_kind", "pent_val")
OUT_KEYS = ("alloc", "avail", "has", "sched_nodes")


def byte_model(a):
    K, R = len(a["cl_node_off"]) - 1, a["n_res"]
    N, P, EN, EP = len(a["node_flags"]), len(a["pod_flags"]), len(a["nent_val"]), len(a["pent_val"])
    node = {"entry_columns": 9 * EN, "offsets": 8 * (N + 1) + 8 * (K + 1), "flags": N, "outputs": 16 * K * R + 16 * K}
    pod = {"entry_columns": 10 * EP, "offsets": 8 * (P + 1) + 8 * (K + 1), "flags": P,
           "outputs": 8 * K * R + 8 * K * R + 8 * K}  # alloc and has read, avail written
    return node, pod


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
        r = ctx.cluster_resources(**a)
        if i >= warmup:
            times.append(ctx.cstat_timing())
    return np.median(np.array(times), axis=0), r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clusters", type=int, default=1000)
    ap.add_argument("--nodes-median", type=float, default=300.0)
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--alternatives", action="store_true")
    a = ap.parse_args()
    import torch  # noqa: F401

    from kubeadmiral_amd import clusterstatus as CS
    from kubeadmiral_amd import runtime, synth

    ctx = runtime.Context(0)
    arr, _, _ = synth.gen_cluster_status(0, a.clusters, nodes_median=a.nodes_median)
    t, r = measure(ctx, arr, a.runs, a.warmup)
    node_b, pod_b = byte_model(arr)
    floor = [sum(node_b.values()) / HBM_ACHIEVABLE * 1e3, sum(pod_b.values()) / HBM_ACHIEVABLE * 1e3]
    t0 = time.perf_counter()
    ref = CS.cstat_numpy(**arr)
    numpy_ms = (time.perf_counter() - t0) * 1e3
    equal = lambda x: all((x[k] == ref[k]).all() for k in OUT_KEYS)  # noqa: E731
    out = {"clusters": a.clusters, "nodes": len(arr["node_flags"]), "pods": len(arr["pod_flags"]),
           "node_entries": len(arr["nent_val"]), "pod_entries": len(arr["pent_val"]), "counter_run": False,
           "node_ms": round(float(t[0]), 4), "pod_ms": round(float(t[1]), 4),
           "h2d_ms_pageable_torch": round(h2d_ms(arr, 3), 3), "node_bytes": node_b, "pod_bytes": pod_b,
           "node_ms_at_hbm": round(floor[0], 4), "pod_ms_at_hbm": round(floor[1], 4),
           "node_ratio": round(float(t[0]) / floor[0], 1), "pod_ratio": round(float(t[1]) / floor[1], 1),
           "total_ratio": round(float(t[0] + t[1]) / (floor[0] + floor[1]), 1),
           "numpy_single_thread_ms": round(numpy_ms, 1), "equals_numpy": equal(r), "route": ctx.cstat_last_route()}
    if a.alternatives:
        alt = {}
        for w, lm in [(w, 0) for w in (8, 16, 32, 64)] + [(0, lm) for lm in (1024, 16384, 65536)]:
            ctx.cstat_debug_route(w, lm)
            t, r2 = measure(ctx, arr, max(3, a.runs // 2), 1)
            route = ctx.cstat_last_route()
            alt[f"width_{w}" if w else f"long_min_{lm}"] = {
                "node_ms": round(float(t[0]), 4), "pod_ms": round(float(t[1]), 4), "long_grid": route["long_grid"],
                "chunk_grid": route["chunk_grid"], "equal": equal(r2)}
        ctx.cstat_debug_route(0, 0)
        out["alternatives"] = alt
    print(json.dumps(out))


if __name__ == "__main__":
    main()
