#!/usr/bin/env python3
"""Device time of one kad_status_aggregate on the scale of the c3 bench workload.

    python scripts/statusagg_cost.py [--config c3] [--objects N] [--runs 10] [--warmup 2] [--alternatives]

synth.gen_status_aggregation makes one source object per unit of the config (1M at c3), each on 1-5 member clusters
and one in 2000 a Duplicate-mode workload on every cluster, for both kinds. kad_sagg_timing's HIP events give the
kernel per call (medians of ``runs``). Beside it stand: the host-to-device time of the same arrays as its own
figure (pageable host memory, through torch); the bytes that must move — segment columns (4 B a summed value, 1 B
of flags, two int64 columns), object columns (offset 4, flags 1, the old status 8 B a row, generation and observed
generation for a Deployment), outputs — and their time at the HBM rate measured as achievable on an MI355X
(6.3 TB/s); the ratio of kernel time to that byte time; and, for comparison only, statusagg.sagg_numpy, a
single-thread numpy restatement on the same arrays. ``--alternatives``: the Deployment workload again under every
group width and, with a hundredth as many objects on 100-2000 clusters each, under other long_min values
(kad_sagg_debug_route). Prints one JSON line."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_ACHIEVABLE = 6.3e12  # B/s


def byte_model(a):
    dep = a["kind"] == 0
    O, S = len(a["obj_flags"]), len(a["seg_flags"])
    nv, nold = (5, 6) if dep else (3, 5)
    return {"segment_columns": S * (4 * nv + 1 + 16), "object_columns": O * (4 + 1 + 8 * nold + (16 if dep else 0)),
            "outputs": O * (4 * nv + 1 + (8 if dep else 25))}


def h2d_ms(a, runs):
    import torch
    ts = []
    for _ in range(runs):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        keep = [torch.from_numpy(np.ascontiguousarray(v)).cuda() for v in a.values() if isinstance(v, np.ndarray) and v.size]
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
        del keep
    return float(np.median(ts))


def measure(ctx, a, runs, warmup):
    times = []
    for i in range(warmup + runs):
        r = ctx.status_aggregate(**a)
        if i >= warmup:
            times.append(ctx.sagg_timing()[0])
    return float(np.median(times)), r


def equal(r, ref):
    return all((np.asarray(r[k]) == np.asarray(ref[k])).all() for k in ref)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="c3")
    ap.add_argument("--objects", type=int, default=0)
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--alternatives", action="store_true")
    a = ap.parse_args()
    import torch  # noqa: F401

    from kubeadmiral_amd import runtime, synth
    from kubeadmiral_amd import statusagg as SA

    W0, C = synth.SIZES[a.config]
    W = a.objects or W0
    ctx = runtime.Context(0)
    out = {"config": a.config, "objects": W, "clusters": C, "counter_run": False}
    for name, kind in (("deployment", SA.DEPLOYMENT), ("job", SA.JOB)):
        arr, _ = synth.gen_status_aggregation(0, kind, W, C)
        t, r = measure(ctx, arr, a.runs, a.warmup)
        b = byte_model(arr)
        floor = sum(b.values()) / HBM_ACHIEVABLE * 1e3
        t0 = time.perf_counter()
        ref = SA.sagg_numpy(**arr)
        numpy_ms = (time.perf_counter() - t0) * 1e3
        out[name] = {"segments": len(arr["seg_flags"]), "changed": int(r["changed"].sum()), "kernel_ms": round(t, 4),
                     "h2d_ms_pageable_torch": round(h2d_ms(arr, 3), 3), "bytes": b, "ms_at_hbm": round(floor, 4),
                     "ratio": round(t / floor, 1), "numpy_single_thread_ms": round(numpy_ms, 1), "equals_numpy": equal(r, ref),
                     "route": ctx.sagg_last_route()}
        if kind == SA.DEPLOYMENT and a.alternatives:
            alt = {}
            for w in (1, 2, 4, 8, 16, 32, 64):
                ctx.sagg_debug_route(w, 0)
                t, r2 = measure(ctx, arr, a.runs, a.warmup)
                alt[f"width_{w}"] = {"kernel_ms": round(t, 4), "equal": equal(r2, ref)}
            # the same batch without its long objects (every object on 1-5 clusters): the width alone
            short, _ = synth.gen_status_aggregation(0, kind, W, C, duplicate_share=0.0)
            refs = SA.sagg_numpy(**short)
            for w in (1, 2, 4, 8):
                ctx.sagg_debug_route(w, 0)
                t, r2 = measure(ctx, short, a.runs, a.warmup)
                alt[f"short_width_{w}"] = {"kernel_ms": round(t, 4), "equal": equal(r2, refs)}
            ctx.sagg_debug_route(0, 0)
            # objects on many clusters for long_min: a hundredth as many objects on 100-2000 clusters each
            rng = np.random.default_rng(1)
            n = max(1, W // 100)
            off = np.zeros(n + 1, np.int64)
            off[1:] = np.cumsum(rng.integers(100, 2001, n))
            big, _ = synth.gen_status_aggregation(1, kind, n, 1 << 30, place_off=off, place_cluster=np.zeros(0, np.int64),
                                                  duplicate_share=0.0)
            refb = SA.sagg_numpy(**big)
            for lm in (64, 128, 256, 512, 1024, 1 << 30):
                ctx.sagg_debug_route(0, lm)
                t, r2 = measure(ctx, big, a.runs, a.warmup)
                route = ctx.sagg_last_route()
                alt[f"long_min_{lm}"] = {"kernel_ms": round(t, 4), "long_grid": route["long_grid"], "width": route["width"],
                                         "segments": len(big["seg_flags"]), "equal": equal(r2, refb)}
            ctx.sagg_debug_route(0, 0)
            out["alternatives"] = alt
    print(json.dumps(out))


if __name__ == "__main__":
    main()
