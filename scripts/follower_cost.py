#!/usr/bin/env python3
"""Device time of one kad_follower_union over the resident results of a scheduled bench workload.

    python scripts/follower_cost.py [--config c3] [--units N] [--per-leader 2.0] [--runs 10] [--warmup 2]

The batch is built as bench.py builds it (same seeds) and scheduled once. Its units are the leaders (resident
mode); synth.gen_followers makes ``per-leader`` followers per leader, each following 1-3 leaders. Two passes
are timed: steady state (1 % of the followers hold a placement that differs from the union) and cold (every
follower holds none, so all change and all emit). kad_follower_timing's HIP events give the union / compare
kernel and the scan + emit per call. Beside them stands the time the bytes that must move would take at the
HBM rate measured as achievable on an MI355X (6.3 TB/s): per leader reference its index (4 B), the unit's
status, count and offsets (4 + 4 + 8 B) and its slots (4 B each); per follower fol_off, cur_off, cur_has and
its current ids (4 + 4 + 1 B, 4 B each), changed, count and out_off written (1 + 4 + 8 B); 4 B per emitted id,
whose leader slots the emit kernel gathers a second time. Prints one JSON line with the medians."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_ACHIEVABLE = 6.3e12  # B/s


def leader_csr(res, batch):
    """The units' placed clusters as a CSR (OK units: their output slots; no-feasible units: none). The
    gathered-slot count and the byte floor rest on it, so a workload with sticky or error-status units, whose
    clusters come from elsewhere, is refused."""
    from kubeadmiral_amd.pack import ST_NO_FEASIBLE, ST_OK

    other = ~np.isin(res.status, (ST_OK, ST_NO_FEASIBLE))
    if other.any():
        raise SystemExit(f"{int(other.sum())} units are sticky or ended in an error: the byte model does not cover them")
    n = np.where(res.status == ST_OK, res.count, 0).astype(np.int64)
    off = np.zeros(len(n) + 1, np.int64)
    off[1:] = np.cumsum(n)
    start = np.repeat(np.asarray(batch.out_off[:-1], np.int64), n)
    within = np.arange(off[-1]) - np.repeat(off[:-1], n)
    return off, res.cluster[start + within].astype(np.int32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="c3")
    ap.add_argument("--units", type=int, default=0)
    ap.add_argument("--per-leader", type=float, default=2.0)
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    a = ap.parse_args()
    import torch  # noqa: F401

    import bench
    from kubeadmiral_amd import columns, runtime, synth
    from kubeadmiral_amd.pack import Snapshot

    W0, C = synth.SIZES[a.config]
    clusters = bench.make_clusters(a.config, C)
    fwk = synth.profile_for(a.config)
    snap = Snapshot(clusters)
    batch = columns.NativePacker(snap).pack(fwk, bench.make_columns(a.config, 0, a.units or W0, clusters))
    ctx = runtime.Context(0)
    ctx.upload_snapshot(snap)
    ctx.upload_batch(batch)
    ctx.schedule(fwk)
    ctx.sync()
    res = ctx.download()
    W = int(batch.W)
    lead_off, lead_cluster = leader_csr(res, batch)
    fol, stale = synth.gen_followers(0, lead_off, lead_cluster, int(snap.C), per_leader=a.per_leader, changed=0.01)
    F = len(fol[4])
    cold = (fol[0], fol[1], np.zeros(F + 1, np.int32), np.zeros(0, np.int32), np.zeros(F, np.uint8))
    n_refs = len(fol[1])
    gathered = int((lead_off[1:] - lead_off[:-1])[fol[1]].sum())  # leader slots read by the union kernel
    out = {"config": a.config, "leaders": W, "clusters": int(snap.C), "followers": F, "leader_refs": n_refs,
           "leader_slots_gathered": gathered, "route": None}
    for name, f in (("steady", fol), ("cold", cold)):
        times, r = [], None
        for i in range(a.warmup + a.runs):
            r = ctx.follower_union(int(snap.C), f, n_leaders=W, capacity=gathered)
            if i >= a.warmup:
                times.append(ctx.follower_timing())
        emitted = int(r["out_off"][-1])
        emit_gather = int(sum((lead_off[1:] - lead_off[:-1])[f[1][f[0][i]:f[0][i + 1]]].sum()
                              for i in np.nonzero(r["changed"])[0])) if name == "steady" else gathered
        b_union = n_refs * (4 + 4 + 4 + 8) + 4 * gathered + F * (4 + 4 + 1) + 4 * len(f[3]) + F * (1 + 4)
        b_emit = F * (1 + 4 + 8) + 4 * emit_gather + 4 * emitted
        t = np.median(np.array(times), axis=0)
        floor = [b_union / HBM_ACHIEVABLE * 1e3, b_emit / HBM_ACHIEVABLE * 1e3]
        out[name] = {"changed": int(r["changed"].sum()), "emitted_ids": emitted, "calls": r["calls"],
                     "union_ms": round(float(t[0]), 4), "scan_emit_ms": round(float(t[1]), 4),
                     "union_bytes": b_union, "scan_emit_bytes": b_emit,
                     "union_ms_at_hbm": round(floor[0], 4), "scan_emit_ms_at_hbm": round(floor[1], 4),
                     "union_ratio": round(float(t[0]) / floor[0], 1), "scan_emit_ratio": round(float(t[1]) / floor[1], 1)}
    out["route"] = ctx.follower_last_route()
    out["stale_followers"] = int(stale.sum())
    again = ctx.download()  # the calls left the schedule's results alone
    out["results_untouched"] = all(getattr(res, k).tobytes() == getattr(again, k).tobytes()
                                   for k in ("status", "count", "flags", "cluster", "replicas"))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
