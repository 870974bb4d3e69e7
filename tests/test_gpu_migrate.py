"""kad_migrate_estimate on an MI355X == the object-by-object checker (migrate_ref.py), exactly: every output is
an integer.

Shapes (migrate_cases.py): segment lengths 0, 1, 7, 8, 9, 63, 64, 65, long_min - 1, long_min, long_min + 1 and
3 * 256 + 5 (long_min read from the route); objects with 0, 1, 2 and 65 segments under every DeepEqual outcome;
crossings of exactly 0 and + 1 ns, a negative threshold, the edges of the time domain, pods without a
transition time, all pods deleting; skipped segments between live ones, a backoff-only object; segments that
alternate long and empty; every group width of the route, forced by the batch's mean segment length."""
import copy

import numpy as np
import pytest

import migrate_cases as MC
import migrate_ref as R
from kubeadmiral_amd import automigration as AM
from kubeadmiral_amd import objects as O
from kubeadmiral_amd import pack, synth

pytestmark = pytest.mark.gpu

KEYS = ("uns", "next_cross", "cap", "changed", "n_written", "retry_after", "backoff")


@pytest.fixture(scope="module")
def ctx():
    from kubeadmiral_amd import build, runtime
    build.build()
    c = runtime.Context(0)
    clusters, _ = synth.gen_fuzz(11, W=1, C=MC.N_IDS - 2)  # two ids past the snapshot's clusters
    c.upload_snapshot(pack.Snapshot(clusters))
    yield c
    c.close()


@pytest.fixture(scope="module")
def long_min():
    from kubeadmiral_amd import runtime
    return runtime.migrate_route_eval(1, 1, 0, 1)["long_min"]


_cases = {}


def shapes(long_min, width):
    """The shapes batch padded with one-pod segments until the route picks ``width``; with its reference."""
    from kubeadmiral_amd import runtime
    if width not in _cases:
        base, _ = MC.shapes_case(long_min)
        S, P = len(base["seg_cluster"]), len(base["pod_t_ns"])
        # mean = (P + pad) / (S + pad) must round up to width: the largest mean that still does
        pad = 0 if width == 64 else max(0, -(-(P - width * S) // (width - 1)))
        arr, marks = MC.shapes_case(long_min, pad_segments=pad)
        n_long = int((np.diff(arr["seg_pod_off"]) > long_min).sum())
        assert runtime.migrate_route_eval(len(arr["seg_cluster"]), len(arr["pod_t_ns"]), n_long,
                                          len(arr["obj_threshold_ns"]))["width"] == width
        _cases[width] = (arr, marks, R.run(**arr))
    return _cases[width]


def assert_equal(got, want):
    for k in KEYS:
        g = [int(x) for x in got[k]]
        assert g == want[k], (k, [i for i, (a, b) in enumerate(zip(g, want[k])) if a != b][:5])


def test_staging_buffer_grows_is_reused_and_shrinks(long_min):
    """One context: a tiny batch with empty parts (an object with zero segments, a segment without pods, no old
    entry, no long segment), the shapes batch (about 100x larger), the tiny one again. Each step equals the
    checker, the third equals the first bit for bit; the timer reports KAD_ESTATE before the first call."""
    from kubeadmiral_amd import runtime
    c = runtime.Context(0)
    try:
        clusters, _ = synth.gen_fuzz(11, W=1, C=3)
        c.upload_snapshot(pack.Snapshot(clusters))
        with pytest.raises(runtime.KadError) as e:
            c.migrate_timing()
        assert e.value.code == runtime.KAD_ESTATE
        b = MC.Builder(n_ids=3)
        U = R.POD_UNSCHED
        b.add(60 * MC.SEC, [], "empty")                                                        # zero segments
        b.add(60 * MC.SEC, [(0, 2, 0, [(U, MC.NOW - 61 * MC.SEC), (U, MC.NOW - 59 * MC.SEC)]), (2, 1, 0, [])], "empty")
        b.add(0, [(1, 3, 0, [(U, MC.NOW), (0, MC.NOW)])], "empty")
        tiny = b.arrays()
        assert len(tiny["old_cluster"]) == 0 and len(tiny["obj_threshold_ns"]) == 3
        want = R.run(**tiny)
        first = c.migrate_estimate(**tiny)
        assert_equal(first, want)
        _timing_ok(c.migrate_timing())
        arr, _, big_want = shapes(long_min, 64)
        assert len(arr["pod_t_ns"]) >= 100 * len(tiny["pod_t_ns"])
        assert_equal(c.migrate_estimate(**arr), big_want)
        _timing_ok(c.migrate_timing())
        again = c.migrate_estimate(**tiny)
        assert_equal(again, want)
        for k in KEYS:
            assert np.asarray(again[k]).tobytes() == np.asarray(first[k]).tobytes(), k
        _timing_ok(c.migrate_timing())
    finally:
        c.close()


def _timing_ok(ms):
    assert len(ms) >= 2 and all(np.isfinite(t) and t >= 0 for t in ms), ms


@pytest.mark.parametrize("width", [64, 32, 16, 8])
def test_shapes_parity(ctx, long_min, width):
    arr, marks, want = shapes(long_min, width)
    got = ctx.migrate_estimate(**arr)
    assert_equal(got, want)
    route = ctx.migrate_last_route()
    assert route["width"] == width and route["long_min"] == long_min
    lens = np.diff(arr["seg_pod_off"])
    assert route["long_grid"] == int(((lens > long_min) & ((arr["seg_flags"] & R.SEG_SKIP) == 0)).sum()) >= 6
    assert set(MC.lengths(long_min)) <= set(lens.tolist())
    # the named shapes say what they were built to say
    o = marks["backoff-only"]
    assert got["backoff"][o] == 1 and got["retry_after"][o] == R.NONE and got["n_written"][o] == 0 and got["changed"][o] == 1
    o = marks["skip-only"]
    assert got["backoff"][o] == 0 and got["retry_after"][o] == R.NONE and got["changed"][o] == 0
    s = arr["obj_seg_off"][marks["exact"]]
    assert got["uns"][s] == 1 and got["next_cross"][s] == 1 and got["cap"][s] == 2
    s = arr["obj_seg_off"][marks["negative-threshold"]]
    assert got["uns"][s] == 2 and got["next_cross"][s] == 1
    s = arr["obj_seg_off"][marks["all-deleting"]]
    assert got["uns"][s] == 0 and got["cap"][s] == -1 and got["cap"][s + 1] == -1
    for old, changed in (("same", 0), ("drop_last", 1), ("alter_last", 1), ("extra", 1)):
        assert got["changed"][marks[f"65-segments-{old}"]] == changed, old
    assert got["changed"][marks["no-segments"]] == 0 and got["changed"][marks["no-segments-stale"]] == 1
    assert all(t >= 0 for t in ctx.migrate_timing())
    # the same batch again on the same context: identical output
    again = ctx.migrate_estimate(**arr)
    for k in KEYS:
        assert (again[k] == got[k]).all(), k


@pytest.mark.parametrize("nseg,width", [(65, 64), (30, 32), (14, 16), (6, 8)])
def test_object_kernel_widths(ctx, nseg, width):
    arr = MC.object_width_case(nseg)
    got = ctx.migrate_estimate(**arr)
    assert ctx.migrate_last_route()["obj_width"] == width
    assert_equal(got, R.run(**arr))
    assert got["changed"][:5].tolist() == [0, 1, 1, 1, 1] and got["n_written"][0] >= 1


@pytest.mark.parametrize("now", [0, MC.TMAX])
def test_time_domain_edges(ctx, now):
    arr = MC.edge_case(now)
    assert_equal(ctx.migrate_estimate(**arr), R.run(**arr))


def test_no_objects_and_invalid(ctx):
    from kubeadmiral_amd import runtime
    empty = MC.Builder().arrays()
    got = ctx.migrate_estimate(**empty)
    assert all(len(got[k]) == 0 for k in KEYS)
    arr = MC.edge_case(0)
    with pytest.raises(runtime.KadError) as e:
        ctx.migrate_estimate(**dict(arr, now_ns=-1))
    assert e.value.code == runtime.KAD_EINVAL
    with pytest.raises(runtime.KadError) as e:
        ctx.migrate_estimate(**dict(arr, n_ids=MC.N_IDS - 3))  # below the snapshot's clusters
    assert e.value.code == runtime.KAD_EINVAL
    fresh = runtime.Context(0)
    try:
        with pytest.raises(runtime.KadError) as e:
            fresh.migrate_estimate(**arr)
        assert e.value.code == runtime.KAD_ESTATE  # no snapshot: C is unknown
        with pytest.raises(runtime.KadError) as e:
            fresh.migrate_timing()
        assert e.value.code == runtime.KAD_ESTATE
    finally:
        fresh.close()


def test_group_member(ctx, long_min):
    from kubeadmiral_amd import runtime
    arr, _, want = shapes(long_min, 64)
    clusters, _ = synth.gen_fuzz(11, W=1, C=MC.N_IDS - 2)
    g = runtime.GroupContext([0, 0])
    try:
        g.upload_snapshot(pack.Snapshot(clusters))
        assert_equal(g.member(1).migrate_estimate(**arr), want)
    finally:
        g.close()


def test_synthetic_batch_against_numpy_and_checker(ctx):
    """A seeded synthetic batch, steady-state and cold: the device == the checker == the numpy restatement."""
    for ready_share in (0.9, 0.0):
        a, stale = synth.gen_migration(7, 700, MC.N_IDS - 2, ready_share=ready_share, extra_ids=2, changed=0.1)
        got = ctx.migrate_estimate(**a)
        assert_equal(got, R.run(**a))
        ref = AM.migrate_numpy(**a)
        for k in KEYS:
            assert (got[k] == ref[k]).all(), k
        assert (got["changed"].astype(bool) == stale).all()


def test_reconcile_auto_migration_end_to_end(ctx):
    """BatchReconciler.reconcile_auto_migration on synth.gen_migration objects == the per-object host path; a
    following reconcile finds the trigger hash of exactly the changed objects changed."""
    from kubeadmiral_amd.controller import BatchReconciler
    rng = np.random.default_rng(3)
    clusters = synth.gen_clusters(rng, 24)
    names = [c.name for c in clusters] + ["left-the-fleet-a", "left-the-fleet-b"]
    a, stale = synth.gen_migration(9, 80, 24, ready_share=0.5, extra_ids=2, changed=0.25, thresholds_s=(60,))
    ftc, objs, cobjs, pods = synth.migration_objects(a, names)
    pol = O.PropagationPolicy("pp", "default", 1, O.PropagationPolicySpec(
        scheduling_mode="Divide", auto_migration=O.AutoMigration(O.AutoMigrationTrigger("1m0s"))))
    for i, obj in enumerate(objs):
        obj["metadata"]["labels"] = {O.PROPAGATION_POLICY_NAME_LABEL: "pp"}
    # objects 0 and 1 are disabled: no threshold / one that does not parse; 0 holds a stale annotation
    del objs[0]["metadata"]["annotations"][O.POD_UNSCHEDULABLE_THRESHOLD_ANNOTATION]
    objs[0]["metadata"]["annotations"][O.AUTO_MIGRATION_INFO_ANNOTATION] = '{"estimatedCapacity":{"x":1}}'
    objs[1]["metadata"]["annotations"][O.POD_UNSCHEDULABLE_THRESHOLD_ANNOTATION] = "later"
    objs[1]["metadata"]["annotations"].pop(O.AUTO_MIGRATION_INFO_ANNOTATION, None)
    policies = {("default", "pp"): pol}
    rec = BatchReconciler(ftc, ctx=ctx)
    first = rec.reconcile(objs, policies, clusters)
    assert all(o.status == "AllOK" for o in first) and sum(o.stage == "scheduled" for o in first) > 40
    # the scheduler wrote the policy's threshold onto the objects it scheduled: 0 and 1 are disabled again
    for o in objs[:2]:
        o["metadata"]["annotations"].pop(O.POD_UNSCHEDULABLE_THRESHOLD_ANNOTATION, None)
    assert all(o.stage == "unchanged" for o in rec.reconcile(objs, policies, clusters))
    host = copy.deepcopy(objs)
    want = [AM.reconcile_object(ftc, o, c, p, a["now_ns"]) for o, c, p in zip(host, cobjs, pods)]
    got = rec.reconcile_auto_migration(objs, cobjs, pods, a["now_ns"])
    assert got == want
    assert objs == host
    assert got[0] == (None, None, True) and got[1] == (None, None, False)
    updated = [g[2] for g in got]
    assert 5 < sum(updated) < len(objs) - 5
    # nothing is left to write
    assert not any(g[2] for g in rec.reconcile_auto_migration(objs, cobjs, pods, a["now_ns"]))
    after = rec.reconcile(objs, policies, clusters)
    for i, o in enumerate(after):
        assert (o.stage != "unchanged") == updated[i], i
    ctx.upload_snapshot(pack.Snapshot(synth.gen_fuzz(11, W=1, C=MC.N_IDS - 2)[0]))  # the module's snapshot again
