#!/usr/bin/env python3
"""What kad_policyrc_count costs: the count kernel on each of its two paths against the bytes it has to read, and
against numpy's histogram of the same ids on the host.

    python scripts/policyrc_cost.py [--ids 1000000,16000000] [--repeat 5] [--events 200000]

For every number of ids (half of them removals, half additions), every table size P of 1 000, the bins limit of the
LDS-private path and 1 000 000, and every id pattern — uniform, grouped in runs of 64 (a batch that arrives grouped
by namespace, hence by policy) and all on one policy — the call runs ``repeat`` times after one warm-up on each path
that is legal for P (kad_policyrc_debug_route). One JSON line a row: the medians of kad_policyrc_timing's intervals
(inputs to the device, the zeroing and prc_count_kernel, prc_apply_kernel), the time the id bytes take at the HBM
rate a streaming kernel sustains on an MI355X, and np.bincount's time on the two lists. The last line splits one
reconcile_policy_refcounts-sized batch of ``events`` object events into the host's interning and packing
(PolicyRefCounter.observe / arrays), the call and apply.
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


def ids_of(np, pattern, n, P, seed):
    if pattern == "uniform":
        return np.random.default_rng(seed).integers(0, P, n).astype(np.int32)
    if pattern == "runs":
        return ((np.arange(n) // 64 + seed) % P).astype(np.int32)
    return np.full(n, P // 2, np.int32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ids", default="1000000,16000000")
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--events", type=int, default=200_000)
    args = ap.parse_args()
    import numpy as np

    from kubeadmiral_amd import build, objects, policyrc, runtime
    build.build()
    ctx = runtime.Context(0)
    bins = runtime.policyrc_route_eval(1, 1)["bins"]
    med = lambda v: round(statistics.median(v), 4)  # noqa: E731
    for n in (int(x) for x in args.ids.split(",")):
        for P in (1000, bins, 1_000_000):
            z = np.zeros(P, np.int64)
            for pattern in ("uniform", "runs", "one"):
                dec, inc = ids_of(np, pattern, n // 2, P, 1), ids_of(np, pattern, n - n // 2, P, 2)
                arr = {"dec_ids": dec, "inc_ids": inc, "count": np.bincount(dec, minlength=P).astype(np.int64),
                       "stored_typed": z, "stored_rest": z, "stored_total": z, "pol_flags": np.full(P, 1, np.uint8)}
                t0 = time.perf_counter()
                want = np.bincount(inc, minlength=P) - np.bincount(dec, minlength=P)
                bincount_ms = (time.perf_counter() - t0) * 1e3
                for force in ((1, 2) if P <= bins else (2,)):
                    ctx.policyrc_debug_route(force)
                    got = ctx.policyrc_count(**arr)
                    assert (got["new_count"] == arr["count"] + want).all() and got["n_negative"][0] == 0
                    h2d, count, apply, wall = [], [], [], []
                    for _ in range(args.repeat):
                        t0 = time.perf_counter()
                        ctx.policyrc_count(**arr)
                        wall.append((time.perf_counter() - t0) * 1e3)
                        ms = ctx.policyrc_timing()
                        h2d.append(ms[0])
                        count.append(ms[1])
                        apply.append(ms[2])
                    route = ctx.policyrc_last_route()
                    print(json.dumps({"ids": n, "P": P, "pattern": pattern, "path": runtime.POLICYRC_PATHS[route["path"]],
                                      "own": runtime.policyrc_route_eval(P, n)["path"] == route["path"], "grid": route["grid"],
                                      "h2d_ms": med(h2d), "count_ms": med(count), "apply_ms": med(apply),
                                      "call_wall_ms": med(wall), "id_byte_ms": round(4 * n / HBM_BYTES_PER_S * 1e3, 4),
                                      "bincount_ms": round(bincount_ms, 2)}), flush=True)
    ctx.policyrc_debug_route(0)
    # the host's share of one reconcile-sized batch: objects of 1000 namespaces x 8 policies each
    E = args.events
    ftc = objects.FederatedTypeConfig("apps", "v1", "Deployment", "deployments", "Namespaced")
    events = [(f"ns{i % 1000}/o{i}", {"metadata": {"name": f"o{i}", "namespace": f"ns{i % 1000}", "labels": {
        objects.PROPAGATION_POLICY_NAME_LABEL: f"p{(i // 1000) % 8}"}}}) for i in range(E)]
    counter = policyrc.PolicyRefCounter(ftc)
    t = [time.perf_counter()]
    counter.observe(events)
    t.append(time.perf_counter())
    arrays = counter.arrays({})
    t.append(time.perf_counter())
    result = ctx.policyrc_count(**arrays)
    t.append(time.perf_counter())
    counter.apply(result, {})
    t.append(time.perf_counter())
    ms = ctx.policyrc_timing()
    print(json.dumps({"events": E, "policies": len(counter.keys), "observe_ms": round((t[1] - t[0]) * 1e3, 1),
                      "arrays_ms": round((t[2] - t[1]) * 1e3, 1), "call_wall_ms": round((t[3] - t[2]) * 1e3, 2),
                      "apply_ms": round((t[4] - t[3]) * 1e3, 1), "device_ms": [round(m, 4) for m in ms]}))
    ctx.close()


if __name__ == "__main__":
    main()
