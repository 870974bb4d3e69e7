#!/usr/bin/env python3
"""Device time of one kad_explain over the KAD_ST_NO_FEASIBLE units of a bench workload, next to the schedule's
own stage times on the same batch.

    python scripts/explain_cost.py [--config c3] [--units N] [--runs 20] [--warmup 3]

The batch is built as bench.py builds it (same seeds). One schedule finds the units without a feasible
cluster; kad_explain then runs over exactly those, without the per-cluster output, and kad_explain_timing's
HIP events give the time of filter_explain_kernel and of the requirement rows' rebuild per call. Prints one
JSON line: the medians, the number of units explained, and the median stage times of the schedule."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="c3")
    ap.add_argument("--units", type=int, default=0)
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    import torch  # noqa: F401

    import bench
    from kubeadmiral_amd import columns, runtime, synth
    from kubeadmiral_amd.pack import ST_NO_FEASIBLE, Snapshot

    W0, C = synth.SIZES[a.config]
    clusters = bench.make_clusters(a.config, C)
    fwk = synth.profile_for(a.config)
    snap = Snapshot(clusters)
    batch = columns.NativePacker(snap).pack(fwk, bench.make_columns(a.config, 0, a.units or W0, clusters))
    ctx = runtime.Context(0)
    ctx.upload_snapshot(snap)
    ctx.upload_batch(batch)
    ctx.set_timing(True)
    stages = []
    for i in range(a.warmup + a.runs):
        ctx.schedule(fwk)
        ctx.sync()
        if i >= a.warmup:
            stages.append(ctx.stage_timing())
    res = ctx.download()
    units = np.nonzero(res.status == ST_NO_FEASIBLE)[0].astype(np.int32)
    rows, kern = [], []
    d = None
    for i in range(a.warmup + a.runs):
        d = ctx.explain(fwk, units)
        if i >= a.warmup and len(units):
            t = ctx.explain_timing()
            rows.append(t[0])
            kern.append(t[1])
    assert d is not None and (d.feasible == 0).all()  # the schedule found no feasible cluster for these
    again = ctx.download()  # the explain calls left the schedule's results alone
    same = all(getattr(res, k).tobytes() == getattr(again, k).tobytes()
               for k in ("status", "count", "flags", "cluster", "replicas"))
    med = lambda v: round(float(np.median(v)), 5) if v else None  # noqa: E731
    print(json.dumps({
        "config": a.config, "units": int(batch.W), "clusters": int(snap.C), "no_feasible_units": int(len(units)),
        "explain_kernel_ms": med(kern), "explain_req_rows_ms": med(rows),
        "rejected_by_plugin": d.rejected.sum(0).tolist(), "fit_detail": d.fit_detail.sum(0).tolist(),
        "first_message": d.message(0) if len(units) else None, "results_unchanged": same,
        "schedule_stage_ms": {k: med([s[k] for s in stages]) for k in stages[0]}}))
    ctx.close()


if __name__ == "__main__":
    main()
