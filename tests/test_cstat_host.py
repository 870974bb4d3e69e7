"""Cluster status on the host: clusterstatus.py against the reference's own table (tests/golden/
federatedcluster.json, Test_aggregateResources) and the independent checker (cstat_ref.py), the number domain and
the host fallback, kad_cstat_check's rules and the route's boundaries. No GPU."""
import copy
import json
import os
from fractions import Fraction

import numpy as np
import pytest

import cstat_cases as CC
import cstat_ref as R
from kubeadmiral_amd import clusterstatus as CS
from kubeadmiral_amd import k8s, pack, runtime, synth
from kubeadmiral_amd import types as T

HERE = os.path.dirname(os.path.abspath(__file__))
with open(os.path.join(HERE, "golden", "federatedcluster.json")) as f:
    GOLDEN = json.load(f)["cases"]


@pytest.fixture(scope="module", autouse=True)
def library():
    from kubeadmiral_amd import build
    build.build()


def by_value(m):
    return {n: R.qty(q) if isinstance(q, str) else Fraction(q) for n, q in m.items()}


def node(alloc=None, spec=None, conditions=None):
    n = {"spec": spec or {}, "status": {"allocatable": alloc or {"cpu": "1"}}}
    if conditions is not None:
        n["status"]["conditions"] = conditions
    return n


def pod(containers=(), init=(), overhead=None, phase="Running"):
    spec = {"containers": [{"resources": {"requests": dict(c)}} for c in containers],
            "initContainers": [{"resources": {"requests": dict(c)}} for c in init]}
    if overhead is not None:
        spec["overhead"] = dict(overhead)
    return {"spec": spec, "status": {"phase": phase}}


def batch_numpy(nodes, pods):
    """One cluster through ClusterStatusBatch's arrays and the numpy restatement: (count, alloc, avail)."""
    b = CS.ClusterStatusBatch()
    b.add(nodes, pods)
    a = b.arrays()
    assert b.device == [0] and not b.host
    assert runtime.cstat_check(**a) == 0
    return b.results(CS.cstat_numpy(**a))[0]


# ------------------------------------------------------------------ the reference's table
@pytest.mark.parametrize("case", GOLDEN, ids=[c["name"] for c in GOLDEN])
def test_golden(case):
    assert len(GOLDEN) == 4
    want_alloc, want_avail = by_value(case["expectedAllocatable"]), by_value(case["expectedAvailable"])
    alloc, avail = CS.aggregate_resources(case["nodes"], case["pods"])
    assert alloc == want_alloc and avail == want_avail
    n, alloc, avail = R.aggregate(case["nodes"], case["pods"])
    assert (n, alloc, avail) == (2, want_alloc, want_avail)
    n, alloc, avail = batch_numpy(case["nodes"], case["pods"])
    assert (n, alloc, avail) == (2, want_alloc, want_avail)


NODE_TABLE = [
    ("plain", node(), True),
    ("cordoned", node(spec={"unschedulable": True}), False),
    ("NoSchedule", node(spec={"taints": [{"key": "k", "effect": "NoSchedule"}]}), False),
    ("NoExecute", node(spec={"taints": [{"key": "k", "effect": "NoExecute"}]}), False),
    ("PreferNoSchedule", node(spec={"taints": [{"key": "k", "effect": "PreferNoSchedule"}]}), True),
    ("ready-true", node(conditions=[{"type": "Ready", "status": "True"}]), True),
    ("ready-false", node(conditions=[{"type": "Ready", "status": "False"}]), False),
    ("ready-unknown", node(conditions=[{"type": "Ready", "status": "Unknown"}]), False),
    ("ready-absent", node(conditions=[{"type": "MemoryPressure", "status": "False"}]), True),
    ("no-conditions", node(conditions=[]), True),
]


@pytest.mark.parametrize("name,n,want", NODE_TABLE, ids=[t[0] for t in NODE_TABLE])
def test_is_node_schedulable(name, n, want):
    assert CS.is_node_schedulable(n) is want
    assert R.node_ok(n) is want


POD_TABLE = [
    ("init-only-name", pod([{"cpu": "1"}], [{"gpu": "2"}, {"gpu": "1"}]), {"cpu": 1, "gpu": 2}),
    ("overhead-only-name", pod([{"cpu": "1"}], overhead={"memory": "64Mi"}), {"cpu": 1, "memory": 64 << 20}),
    ("init-smaller", pod([{"cpu": "300m"}, {"cpu": "300m"}], [{"cpu": "500m"}]), {"cpu": Fraction(3, 5)}),
    ("init-larger", pod([{"cpu": "300m"}, {"cpu": "300m"}], [{"cpu": "100m"}, {"cpu": "2"}]), {"cpu": 2}),
    ("init-then-overhead", pod([{"cpu": "1"}], [{"cpu": "3"}], {"cpu": "250m"}), {"cpu": Fraction(13, 4)}),
    ("nothing", pod(), {}),
]


@pytest.mark.parametrize("name,p,want", POD_TABLE, ids=[t[0] for t in POD_TABLE])
def test_pod_resource_requests(name, p, want):
    want = {n: Fraction(v) for n, v in want.items()}
    assert CS.pod_resource_requests(p) == want
    assert R.pod_requests(p) == want
    # through the batch: a node that offers every name, so the request shows in Available
    offer = node({n: "100" for n in ("cpu", "memory", "gpu")})
    _, alloc, avail = batch_numpy([offer], [p])
    assert {n: alloc[n] - avail[n] for n in alloc if alloc[n] != avail[n]} == want


def three_ways(nodes, pods):
    got = CS.cluster_resources(nodes, pods)
    assert got == R.aggregate(nodes, pods)
    assert batch_numpy(nodes, pods) == got
    return got


def test_aggregation_rules():
    # a name present at value 0; pods dropped; a request for a name no schedulable node lists is ignored
    n, alloc, avail = three_ways([node({"cpu": "2", "gpu": "0", "pods": "110"}),
                                  node({"cpu": "1", "fpga": "4"}, spec={"unschedulable": True})],
                                 [pod([{"cpu": "500m", "gpu": "1", "fpga": "1", "pods": "1"}])])
    assert n == 1 and alloc == {"cpu": 2, "gpu": 0} and avail == {"cpu": Fraction(3, 2), "gpu": -1}
    # all nodes unschedulable: empty lists, count 0
    assert three_ways([node(spec={"unschedulable": True}), node(conditions=[{"type": "Ready", "status": "False"}])],
                      [pod([{"cpu": "1"}])]) == (0, {}, {})
    # terminal pods are skipped
    n, alloc, avail = three_ways([node({"cpu": "4"})], [pod([{"cpu": "1"}], phase="Succeeded"),
                                                        pod([{"cpu": "1"}], phase="Failed"),
                                                        pod([{"cpu": "1"}], phase="Pending"), pod([{"cpu": "1"}], phase="")])
    assert avail == {"cpu": 2}
    # negative Available
    n, alloc, avail = three_ways([node({"cpu": "1", "memory": "1Gi"})], [pod([{"cpu": "1500m", "memory": "3Gi"}])] * 2)
    assert avail == {"cpu": -2, "memory": -5 * (1 << 30)}
    assert three_ways([], []) == (0, {}, {})


@pytest.mark.parametrize("text,scale,scaled", [("100m", 3, 100), ("1n", 9, 1), ("0.5", 3, 500), ("1.5Gi", 0, 1610612736),
                                               ("1e3", 0, 1000), ("0", 0, 0), ("1500u", 6, 1500), ("2500m", 3, 2500)])
def test_scale_choice(text, scale, scaled):
    q = k8s.quantity(text)
    assert q == R.qty(text)
    assert CS.scale_of(q) == scale
    b = CS.ClusterStatusBatch()
    b.add([node({"x": text, "y": "7"})], [])
    a = b.arrays()
    assert b.scales == [scale, 0] and a["nent_val"].tolist() == [scaled, 7]
    assert k8s.quantity(CS.format_quantity(q)) == q


def test_column_scale_is_the_finest_of_the_call():
    b = CS.ClusterStatusBatch()
    b.add([node({"cpu": "2"})], [pod([{"cpu": "100m"}])])
    b.add([node({"cpu": "1"})], [pod([{"cpu": "1n"}])])
    a = b.arrays()
    assert b.scales == [9] and a["nent_val"].tolist() == [2 * 10**9, 10**9] and a["pent_val"].tolist() == [10**8, 1]
    got = b.results(CS.cstat_numpy(**a))
    assert got[1] == (1, {"cpu": 1}, {"cpu": 1 - Fraction(1, 10**9)})
    assert CS.format_quantity(got[1][2]["cpu"]) == "999999999n" and CS.format_quantity(got[0][2]["cpu"]) == "1900m"


def many_names(n):
    return node({f"example.com/r{i}": "1" for i in range(n)})


FALLBACK = [
    (CS.HOST_NEGATIVE, [node({"cpu": "4"})], [pod([{"cpu": "-1"}])]),
    (CS.HOST_NEGATIVE, [node({"cpu": "-4"})], []),
    (CS.HOST_BOUND, [node({"memory": "8Ei", "cpu": "1n"})], [pod([{"cpu": "1"}])]),
    (CS.HOST_BOUND, [node({"cpu": "1"})], [pod([{"cpu": str(1 << 60)}] * 5)]),
    (CS.HOST_NAMES, [node({"cpu": "1"}), many_names(70)], [pod([{"example.com/r69": "1"}])]),
]


@pytest.mark.parametrize("reason,nodes,pods", FALLBACK, ids=[f"{t[0]}-{i}" for i, t in enumerate(FALLBACK)])
def test_out_of_domain_reaches_the_host_fallback(reason, nodes, pods):
    """The affected cluster is computed on the host, exactly; its neighbours stay on the device path and the
    call's arrays pass the library's validation."""
    plain_nodes, plain_pods = [node({"cpu": "2", "memory": "1Gi"})], [pod([{"cpu": "250m"}])]
    b = CS.ClusterStatusBatch()
    b.add(plain_nodes, plain_pods)
    b.add(nodes, pods)
    b.add(plain_nodes, plain_pods)
    a = b.arrays()
    assert b.host == {1: reason} and b.device == [0, 2]
    assert 1 <= a["n_res"] <= 64 and len(a["cl_node_off"]) == 3
    assert runtime.cstat_check(**a) == 0
    got = b.results(CS.cstat_numpy(**a))
    assert got[1] == R.aggregate(nodes, pods)
    assert got[0] == got[2] == R.aggregate(plain_nodes, plain_pods)


def test_every_cluster_on_the_host():
    b = CS.ClusterStatusBatch()
    b.add([node({"cpu": "-1"})], [])
    a = b.arrays()
    assert b.device == [] and runtime.cstat_check(**a) == 0
    assert b.results(None) == [(1, {"cpu": -1}, {"cpu": -1})]


# ------------------------------------------------------------------ kad_cstat_check
def small_batch():
    b = CC.Builder(3)
    b.add([(1, [(0, 5), (2, 7)]), (0, [(1, 1)])], [(0, [(0, 0, 1), (0, 1, 2), (2, 2, 3)]), (1, []), (0, [(1, 0, 4), (1, 0, 5)])])
    b.add([(1, [(1, 9)])], [(0, [(0, 0, 1)])])
    return b.arrays()


def test_check_accepts_the_built_batches():
    assert runtime.cstat_check(**small_batch()) == 0
    assert runtime.cstat_check(**CC.shapes_case(4096)[0]) == 0
    assert runtime.cstat_check(**CC.mixed_case(65, 63, 2)) == 0
    assert runtime.cstat_check(**CC.bound_case()) == 0
    assert runtime.cstat_check(**CC.Builder(1).arrays()) == 0  # K = 0
    a, _, _ = synth.gen_cluster_status(3, 12, nodes_median=20)
    assert runtime.cstat_check(**a) == 0


def mutate(a, key, index, value):
    a = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in a.items()}
    if key == "n_res":
        a[key] = value
    else:
        a[key][index] = value
    return a


MUTATIONS = [
    ("cl_node_off", 1, 4), ("cl_node_off", 0, 1), ("node_ent_off", 1, 4), ("cl_pod_off", 1, 5), ("pod_ent_off", 2, 2),
    ("pod_ent_off", 4, 7),                 # offsets: non-monotone, not from 0, not ending at the count
    ("nent_res", 0, 3), ("pent_res", 5, 3),  # a resource id >= R
    ("pent_kind", 0, 3),                   # a bad kind
    ("pent_kind", 0, 2), ("pent_res", 0, 2),  # unsorted entries: by kind within a resource, by resource
    ("nent_val", 1, -1), ("pent_val", 2, -1),  # a negative value
    ("nent_val", 0, (1 << 61) + 1), ("pent_val", 0, (1 << 62) // 3 + 1),  # the overflow bound (3 / 5 entries a cluster)
    ("node_flags", 0, 2), ("pod_flags", 0, 3),  # an unknown flag
    ("n_res", None, 0), ("n_res", None, 65), ("n_res", None, 2),
]


@pytest.mark.parametrize("key,index,value", MUTATIONS, ids=[f"{k}-{i}-{j}" for j, (k, i, _) in enumerate(MUTATIONS)])
def test_check_rejects_one_mutation_of_each_rule(key, index, value):
    assert runtime.cstat_check(**mutate(small_batch(), key, index, value)) == runtime.KAD_EINVAL


def test_check_bound_is_exact():
    a = small_batch()  # at most 3 node entries and 5 pod entries in one cluster
    ok = mutate(mutate(a, "nent_val", 0, (1 << 62) // 3), "pent_val", 0, (1 << 62) // 5)
    assert runtime.cstat_check(**ok) == 0
    assert runtime.cstat_check(**mutate(ok, "nent_val", 0, (1 << 62) // 3 + 1)) == runtime.KAD_EINVAL
    assert runtime.cstat_check(**mutate(ok, "pent_val", 0, (1 << 62) // 5 + 1)) == runtime.KAD_EINVAL


# ------------------------------------------------------------------ the route
def test_route_width_and_long_min_boundaries():
    ev = runtime.cstat_route_eval
    base = ev(1, 0, 1, 1, 0)
    long_min = base["long_min"]
    assert long_min >= 64 and base["threads"] == 256 and base["node_width"] == base["pod_width"] == 8
    # width = ceil(mean / 8) rounded up to a power of two, clamped to [8, 64]
    for mean, width in ((0, 8), (1, 8), (64, 8), (65, 16), (128, 16), (129, 32), (256, 32), (257, 64), (512, 64),
                        (513, 64), (100000, 64)):
        r = ev(10, 0, 10 * mean, 10, 0)
        assert (r["node_width"], r["pod_width"]) == (width, 8), mean
        r = ev(10, 0, 10, 10 * mean, 0)
        assert (r["node_width"], r["pod_width"]) == (8, width), mean
    # the means are over the short clusters alone
    assert ev(10, 8, 2 * 65, 2, 3)["node_width"] == 16 and ev(10, 8, 2 * 64, 2, 3)["node_width"] == 8
    # grids: one group per cluster up to 8 blocks a CU; the long path's blocks are the caller's counts
    r = ev(1000, 7, 5000, 5000, 19, 256)
    assert r["node_grid"] == r["pod_grid"] == -(-1000 // 32) and r["long_grid"] == 7 and r["chunk_grid"] == 19
    assert ev(10**6, 0, 10**6, 10**6, 0, 4)["node_grid"] == 32
    r = ev(5, 5, 0, 0, 9)
    assert r["node_grid"] == r["pod_grid"] == 0 and r["long_grid"] == 5
    for bad in ((-1, 0, 0, 0, 0), (1, 2, 0, 0, 0), (1, 0, -1, 0, 0), (1, 0, 0, 0, -1)):
        with pytest.raises(ValueError):
            ev(*bad)
    # the counts the tests derive from arrays put long_min - 1 and long_min entries on the group path
    a, marks = CC.shapes_case(long_min)
    assert [CC.entries_of(a, marks[f"entries-{d}"]) - long_min for d in (-1, 0, 1)] == [-1, 0, 1]
    K, n_long, _, _, n_chunks = CC.route_counts(a, long_min)
    assert n_long == 3 and n_chunks >= 3 + 1  # entries-1, the 773-node cluster, the three-chunk cluster


# ------------------------------------------------------------------ apply and the snapshot
def test_apply_round_trip_through_the_snapshot():
    """apply's clusters through pack.Snapshot give the same columns as clusters built from the checker's
    quantities; unchanged clusters are returned as they are."""
    a, names, scales = synth.gen_cluster_status(5, 6, nodes_median=12, pods_per_node=4)
    cluster_nodes, cluster_pods = synth.cluster_status_objects(a, names, scales)
    clusters, _ = synth.gen_fuzz(21, W=1, C=6)
    b = CS.ClusterStatusBatch()
    for n, p in zip(cluster_nodes, cluster_pods):
        b.add(n, p)
    arr = b.arrays()
    assert b.names == list(names) and b.scales == list(scales) and not b.host
    for k in arr:
        assert np.array_equal(arr[k], a[k]), k  # the dicts say what the arrays said
    r = CS.cstat_numpy(**arr)
    want_r = R.run(**arr)
    for k in ("alloc", "avail", "has", "sched_nodes"):
        assert [int(x) for x in r[k]] == want_r[k], k
    objs = [{"metadata": {"name": c.name}} for c in clusters]
    before = copy.deepcopy(clusters)
    new, changed = b.apply(r, clusters, objs)
    assert clusters == before and changed == [c.name for c in clusters]
    want = []
    for c, n, p, o in zip(clusters, cluster_nodes, cluster_pods, objs):
        count, alloc, avail = R.aggregate(n, p)
        want.append(T.FederatedCluster(c.name, c.labels, c.taints, c.api_resource_types,
                                       {k: R.text(v) for k, v in alloc.items()}, {k: R.text(v) for k, v in avail.items()}))
        res = o["status"]["resources"]
        assert res["schedulableNodes"] == count and "pods" not in res["allocatable"]
        assert by_value(res["allocatable"]) == alloc and by_value(res["available"]) == avail
    assert np.array_equal(pack.Snapshot(new).blob, pack.Snapshot(want).blob)
    again, changed = b.apply(r, new, None)
    assert changed == [] and all(x is y for x, y in zip(again, new))
    assert pack.Snapshot(new).diff(again).changed == []
