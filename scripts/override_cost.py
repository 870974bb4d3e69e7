#!/usr/bin/env python3
"""Device time of one kad_override_match over the placements of a scheduled bench workload.

    python scripts/override_cost.py [--config c3] [--units N] [--policies 2000] [--runs 20] [--warmup 3]

The batch is built as bench.py builds it (same seeds) and scheduled once; ~2000 (Cluster)OverridePolicies of
~4 rules (synth.gen_override_policies) are uploaded, every unit gets a cluster-scoped and a namespaced policy,
and kad_override_match runs with the placed clusters taken from the resident results. kad_override_timing's
HIP events give the three stage times per call. Beside the status + match kernels' time stands the time their
compulsory bytes would take at the HBM rate measured as achievable on an MI355X (6.3 TB/s): slot ids read
(4 B per slot) + RW words written per slot + policy ids (8 B) and the offsets and result words that locate an
object's slots (out_off 8 B, cur_off 4 B, status 4 B, count 4 B) per object + the status written (4 B).
Prints one JSON line with the medians."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_ACHIEVABLE = 6.3e12  # B/s


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="c3")
    ap.add_argument("--units", type=int, default=0)
    ap.add_argument("--policies", type=int, default=2000)
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    import torch  # noqa: F401

    import bench
    from kubeadmiral_amd import columns, overrides, runtime, synth
    from kubeadmiral_amd.pack import ST_OK, Snapshot

    W0, C = synth.SIZES[a.config]
    clusters = bench.make_clusters(a.config, C)
    fwk = synth.profile_for(a.config)
    snap = Snapshot(clusters)
    batch = columns.NativePacker(snap).pack(fwk, bench.make_columns(a.config, 0, a.units or W0, clusters))
    pols = synth.gen_override_policies(0, clusters, n_policies=a.policies, max_rules=8, n_keys=8, n_vals=8, n_int_keys=0)
    pset = overrides.PolicySet(snap, pols)
    ctx = runtime.Context(0)
    ctx.upload_snapshot(snap)
    ctx.upload_batch(batch)
    ctx.upload_override_policies(pset)
    ctx.set_timing(True)
    ctx.schedule(fwk)
    ctx.sync()
    stage = ctx.stage_timing()
    res = ctx.download()
    W = int(batch.W)
    rng = np.random.default_rng(0)
    cp = np.array([i for i, p in enumerate(pols) if not p.namespace], np.int32)
    npol = np.array([i for i, p in enumerate(pols) if p.namespace], np.int32)
    op = np.stack([cp[rng.integers(0, len(cp), W)], npol[rng.integers(0, len(npol), W)]], 1).astype(np.int32)
    rw = pset.rule_words(op)
    times = []
    status = rows = None
    for i in range(a.warmup + a.runs):
        status, rows = ctx.override_match(op, None, rule_words=rw)
        if i >= a.warmup:
            times.append(ctx.override_timing())
    again = ctx.download()  # the match calls left the schedule's results alone
    same = all(getattr(res, k).tobytes() == getattr(again, k).tobytes()
               for k in ("status", "count", "flags", "cluster", "replicas"))
    n_slots = len(rows)
    placed = int(res.count[res.status == ST_OK].sum())
    compulsory = n_slots * (4 + 4 * rw) + W * (8 + 8 + 4 + 4 + 4 + 4)
    t = np.median(np.array(times), axis=0)
    floor_ms = compulsory / HBM_ACHIEVABLE * 1e3
    print(json.dumps({
        "config": a.config, "units": W, "clusters": int(snap.C), "policies": pset.P, "rules": pset.R,
        "distinct_requirements": int(len(pset.arrays[overrides.O_REQ_OFF]) - 1), "rule_words": rw, "slots": n_slots,
        "placed_slots_ok_units": placed, "failed_objects": int((status != 0).sum()),
        "matched_bits": int(np.unpackbits(rows.view(np.uint8)).sum()),
        "req_rows_ms": round(float(t[0]), 5), "rule_rows_ms": round(float(t[1]), 5), "match_ms": round(float(t[2]), 5),
        "compulsory_bytes": int(compulsory), "hbm_floor_ms": round(floor_ms, 5),
        "match_over_floor": round(float(t[2]) / floor_ms, 2) if floor_ms else None,
        "results_unchanged": same, "schedule_total_ms": round(stage["total"], 5)}))
    ctx.close()


if __name__ == "__main__":
    main()
