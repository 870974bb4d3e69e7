"""kad_cluster_resources on an MI355X == the entry-by-entry checker (cstat_ref.py), exactly: every output is an
integer.

Shapes (cstat_cases.py): clusters of 0, 1, 63, 64, 65 and 3 * 256 + 5 nodes; long_min - 1, long_min and long_min + 1
entries (long_min read from the route); a long cluster whose pods fill two chunks and one pod more; pods without
entries and pods naming all R names in one run; K of 1, 2, 65 and 257 with R of 1, 63, 64 and 5, short and long
mixed; presence bits 0 and 63 alone; sums of exactly 2^62; every group width, chosen by the route and forced; the
long path forced on short clusters; no schedulable node, every pod terminal, negative Available."""
import copy

import numpy as np
import pytest

import cstat_cases as CC
import cstat_ref as R
from kubeadmiral_amd import clusterstatus as CS
from kubeadmiral_amd import objects as O
from kubeadmiral_amd import pack, synth
from kubeadmiral_amd import types as T
from tests.gpu_util import assert_same, c_oracle

pytestmark = pytest.mark.gpu

KEYS = ("alloc", "avail", "has", "sched_nodes")


@pytest.fixture(scope="module")
def ctx():
    from kubeadmiral_amd import build, runtime
    build.build()
    c = runtime.Context(0)  # no snapshot: the call needs none
    yield c
    c.close()


@pytest.fixture(scope="module")
def long_min():
    from kubeadmiral_amd import runtime
    return runtime.cstat_route_eval(1, 0, 1, 1, 0)["long_min"]


def assert_equal(got, want):
    for k in KEYS:
        g = [int(x) for x in got[k]]
        assert g == want[k], (k, [i for i, (a, b) in enumerate(zip(g, want[k])) if a != b][:5])


def row(r, arr, k, key):
    n = arr["n_res"]
    return [int(x) for x in r[key][k * n:(k + 1) * n]]


def test_shapes_parity_and_route(ctx, long_min):
    from kubeadmiral_amd import runtime
    fresh = runtime.Context(0)
    try:
        with pytest.raises(runtime.KadError) as e:
            fresh.cstat_timing()
        assert e.value.code == runtime.KAD_ESTATE
    finally:
        fresh.close()
    arr, marks = CC.shapes_case(long_min)
    want = R.run(**arr)
    got = ctx.cluster_resources(**arr)
    assert_equal(got, want)
    # last_route equals route_eval for the same counts
    route = ctx.cstat_last_route()
    assert route == runtime.cstat_route_eval(*CC.route_counts(arr, long_min))
    assert route["long_min"] == long_min and route["long_grid"] == 3 and route["chunk_grid"] >= 5
    # the named shapes say what they were built to say
    k = marks["unschedulable"]
    assert got["has"][k] == 0 and got["sched_nodes"][k] == 0 and not any(row(got, arr, k, "alloc") + row(got, arr, k, "avail"))
    k = marks["terminal"]
    assert row(got, arr, k, "avail") == row(got, arr, k, "alloc") == [10, 20, 0, 0, 0]
    k = marks["negative"]
    assert row(got, arr, k, "avail") == [10 - 2 * 13, -8, 0, 0, 0] and got["has"][k] == 3
    k = marks["no-nodes"]
    assert got["has"][k] == 0 and not any(row(got, arr, k, "avail"))
    k = marks["chunks"]
    assert got["sched_nodes"][k] > 0
    ms = ctx.cstat_timing()
    assert len(ms) == 2 and all(np.isfinite(t) and t >= 0 for t in ms)
    again = ctx.cluster_resources(**arr)
    for key in KEYS:
        assert np.asarray(again[key]).tobytes() == np.asarray(got[key]).tobytes(), key


@pytest.mark.parametrize("width", [8, 16, 32, 64])
def test_group_widths_chosen_by_the_route(ctx, width):
    arr = CC.width_case(width)
    got = ctx.cluster_resources(**arr)
    route = ctx.cstat_last_route()
    assert (route["node_width"], route["pod_width"], route["long_grid"]) == (width, width, 0)
    assert_equal(got, R.run(**arr))


_mixed = {}


def mixed(K, R_):
    if (K, R_) not in _mixed:
        arr = CC.mixed_case(K, R_, seed=3)
        _mixed[K, R_] = (arr, R.run(**arr))
    return _mixed[K, R_]


@pytest.mark.parametrize("width", [8, 16, 32, 64])
def test_group_widths_forced(ctx, width):
    arr, want = mixed(65, 5)
    ctx.cstat_debug_route(width, 0)
    try:
        got = ctx.cluster_resources(**arr)
        route = ctx.cstat_last_route()
    finally:
        ctx.cstat_debug_route(0, 0)
    assert (route["node_width"], route["pod_width"]) == (width, width)
    assert_equal(got, want)


@pytest.mark.parametrize("K,R_", [(1, 1), (2, 63), (65, 64), (257, 5)])
def test_cluster_and_resource_counts_short_and_long_mixed(ctx, K, R_):
    """long_min forced to 64: every 16th cluster of the mix is on the long path, the others on the group path."""
    arr, want = mixed(K, R_)
    ctx.cstat_debug_route(0, 64)
    try:
        got = ctx.cluster_resources(**arr)
        route = ctx.cstat_last_route()
    finally:
        ctx.cstat_debug_route(0, 0)
    n_long = sum(CC.entries_of(arr, k) > 64 for k in range(K))
    assert route["long_min"] == 64 and route["long_grid"] == n_long and (n_long > 0) == (K >= 16)
    assert_equal(got, want)
    # and with the route's own long_min: all of them short
    got = ctx.cluster_resources(**arr)
    assert ctx.cstat_last_route()["long_grid"] == 0
    assert_equal(got, want)


def test_long_path_forced_on_short_clusters(ctx):
    arr, want = mixed(65, 5)
    ctx.cstat_debug_route(0, 1)
    try:
        got = ctx.cluster_resources(**arr)
        route = ctx.cstat_last_route()
    finally:
        ctx.cstat_debug_route(0, 0)
    assert route["long_grid"] == sum(CC.entries_of(arr, k) > 1 for k in range(65)) > 55
    assert_equal(got, want)


def test_domain_bound_and_presence_bits(ctx):
    arr = CC.bound_case()
    got = ctx.cluster_resources(**arr)
    assert_equal(got, R.run(**arr))
    assert [int(h) for h in got["has"]] == [1, (1 << 63) | (1 << 5), 1 << 63]
    assert int(got["alloc"][0]) == CC.BOUND and int(got["avail"][0]) == 0
    assert int(got["alloc"][64 + 63]) == 0 and int(got["avail"][64 + 63]) == -CC.BOUND
    assert int(got["avail"][2 * 64 + 63]) == 9 - 3 and int(got["avail"][2 * 64]) == 0


def test_no_clusters_and_invalid(ctx):
    from kubeadmiral_amd import runtime
    got = ctx.cluster_resources(**CC.Builder(3).arrays())
    assert all(len(got[k]) == 0 for k in KEYS)
    arr = CC.bound_case()
    for bad in (dict(arr, n_res=65), dict(arr, nent_val=arr["nent_val"] + 1)):  # R, the overflow bound
        with pytest.raises(runtime.KadError) as e:
            ctx.cluster_resources(**bad)
        assert e.value.code == runtime.KAD_EINVAL


def test_group_member(ctx, long_min):
    from kubeadmiral_amd import runtime
    arr, want = mixed(257, 5)
    g = runtime.GroupContext([0, 0])
    try:
        assert_equal(g.member(1).cluster_resources(**arr), want)
    finally:
        g.close()


def test_synthetic_batch_against_numpy_and_checker(ctx):
    a, _, _ = synth.gen_cluster_status(7, 40, nodes_median=30, pods_per_node=10, max_nodes=600)
    got = ctx.cluster_resources(**a)
    assert_equal(got, R.run(**a))
    ref = CS.cstat_numpy(**a)
    for k in KEYS:
        assert (got[k] == ref[k]).all(), k
    assert ctx.cstat_last_route()["long_grid"] > 0 and ctx.cstat_last_route()["node_grid"] > 0


def test_reconcile_cluster_status_end_to_end(ctx):
    """nodes / pods → resources → snapshot delta → kad_schedule: after reconcile_cluster_status the next
    schedule equals the C oracle on clusters whose resources come from the checker; an unchanged second pass
    uploads nothing; one node losing its readiness changes exactly its cluster, by a delta."""
    from kubeadmiral_amd.controller import BatchReconciler
    C = 20
    a, names, scales = synth.gen_cluster_status(9, C, nodes_median=15, pods_per_node=5, max_nodes=200)
    cluster_nodes, cluster_pods = synth.cluster_status_objects(a, names, scales)
    clusters, units = synth.gen_fuzz(31, W=60, C=C)
    base = copy.deepcopy(clusters)
    fwk = synth.fuzz_framework(3)  # ClusterResourcesFit and the allocation scores read the columns
    ftc = O.FederatedTypeConfig("apps", "v1", "Deployment", "deployments", "Namespaced", "spec.replicas",
                                "status.replicas", "status.readyReplicas")
    rec = BatchReconciler(ftc, ctx=ctx)
    rec.scheduler.set_clusters(clusters)  # the resident snapshot holds invented resources

    def expected():
        out = []
        for c, n, p in zip(base, cluster_nodes, cluster_pods):
            _, alloc, avail = R.aggregate(n, p)
            out.append(T.FederatedCluster(c.name, c.labels, c.taints, c.api_resource_types,
                                          {k: R.text(v) for k, v in alloc.items()}, {k: R.text(v) for k, v in avail.items()}))
        return out

    def check_schedule():
        want_snap = pack.Snapshot(expected())
        want = c_oracle(want_snap, pack.Batch(want_snap, fwk, units), fwk)
        snap = rec.scheduler.set_clusters(clusters)
        assert_same(ctx.run(fwk, pack.Batch(snap, fwk, units)), want, "after reconcile_cluster_status")
        return want

    objs = [{"metadata": {"name": c.name}} for c in clusters]
    changed = rec.reconcile_cluster_status(clusters, cluster_nodes, cluster_pods, objs)
    assert changed == [c.name for c in clusters]
    assert all(o["status"]["resources"]["schedulableNodes"] == R.aggregate(n, p)[0]
               for o, n, p in zip(objs, cluster_nodes, cluster_pods))
    first = check_schedule()
    assert (first.status == pack.ST_OK).sum() > 5
    # unchanged nodes and pods: no cluster changed, nothing uploaded
    before = (rec.scheduler.full_uploads, rec.scheduler.delta_updates)
    held = list(clusters)
    assert rec.reconcile_cluster_status(clusters, cluster_nodes, cluster_pods) == []
    assert (rec.scheduler.full_uploads, rec.scheduler.delta_updates) == before
    assert all(x is y for x, y in zip(clusters, held))
    # one node of cluster 3 loses its readiness
    node = next(n for n in cluster_nodes[3] if CS.is_node_schedulable(n) and len(n["status"]["allocatable"]) > 1)
    node["status"]["conditions"] = [{"type": "Ready", "status": "False"}]
    assert rec.reconcile_cluster_status(clusters, cluster_nodes, cluster_pods) == [clusters[3].name]
    assert (rec.scheduler.full_uploads, rec.scheduler.delta_updates) == (before[0], before[1] + 1)
    check_schedule()
