"""kad_sync_needs_update and kad_sync_finish on an MI355X == the per-object checker (syncfin_ref.py), mapped through
SyncFinishBatch.apply, exactly: every output is an integer or a flag.

The named cases and seeded batches at every lane-group width (forced through kad_sync_finish_debug_route) and on the
block path (long_min forced low); objects of 0, 1, width - 1, width, width + 1 and 2 * width + 1 entries; one object of
a few thousand entries for the carry across passes; C of 1, 64, 65 and 16384; a STATUS_ON_HOST object between device
objects with the share of such objects asserted; a batch twice; a schedule result left alone; a kad_group member."""
import numpy as np
import pytest

import syncfin_cases as SC
import syncfin_ref as R
from kubeadmiral_amd import syncfin as SF

pytestmark = pytest.mark.gpu

WIDTHS = (1, 2, 4, 8, 16, 32, 64)
HEAD = ("n_clusters", "n_reasons", "reason_check_clusters", "reason_ns_not_federated")


@pytest.fixture(scope="module")
def ctx():
    from kubeadmiral_amd import build, runtime
    build.build()
    c = runtime.Context(0)
    yield c
    c.close()


def finish(ctx, batch, width=0, long_min=0):
    a = batch.finish_arrays()
    ctx.sync_finish_debug_route(width, long_min)
    try:
        return ctx.sync_finish(*[a.pop(k) for k in HEAD], **a)
    finally:
        ctx.sync_finish_debug_route(0, 0)


def check(ctx, cl, objs, width=0, long_min=0):
    b = SC.pack(cl, objs)
    res = finish(ctx, b, width, long_min)
    assert SC.compare(b, res, objs) is None
    return b, res


_NAMED = SC.named()


@pytest.mark.parametrize("width", (0,) + WIDTHS)
def test_named_cases_at_every_width(ctx, width):
    for name, (cl, objs) in sorted(_NAMED.items()):
        check(ctx, cl, objs, width)
    # and all of them as one batch: objects of different lengths share a wave
    cl = SC.names(8)
    check(ctx, cl, [o for _, (_, objs) in sorted(_NAMED.items()) for o in objs], width)
    assert width == 0 or ctx.sync_finish_last_route()["width"] == width


def test_named_cases_on_the_block_path(ctx):
    cl = SC.names(8)
    objs = [o for _, (_, objs) in sorted(_NAMED.items()) for o in objs]
    check(ctx, cl, objs, long_min=1)
    r = ctx.sync_finish_last_route()
    assert r["long_min"] == 1 and 0 < r["long_grid"] < len(objs) and r["grid"] > 0


@pytest.mark.parametrize("width", WIDTHS)
def test_list_lengths_around_the_width(ctx, width):
    sizes = sorted({0, 1, width - 1, width, width + 1, 2 * width + 1} - {-1})
    cl, objs = SC.sized_batch(width, 160, sizes * 3)
    check(ctx, cl, objs, width)
    check(ctx, cl, objs, width, long_min=width)  # the longer ones a block each


@pytest.mark.parametrize("C,size", [(1, 1), (64, 64), (65, 65)])
def test_cluster_counts(ctx, C, size):
    cl, objs = SC.random_batch(C, C, 40, size)
    check(ctx, cl, objs)
    check(ctx, cl, objs, 64)


def test_one_long_object_carries_across_passes(ctx):
    """3000 entries: 12 passes of a block, 47 of a 64-lane group; C = 16384."""
    cl, objs = SC.sized_batch(7, 16384, [3000, 5, 2100])
    b, res = check(ctx, cl, objs, long_min=256)
    r = ctx.sync_finish_last_route()
    assert r["long_grid"] == 2 and int(res["ver_count"][0]) > 1024 and int(res["st_count"][0]) > 1024
    b64, res64 = check(ctx, cl, objs, 64, long_min=100000)
    assert ctx.sync_finish_last_route()["long_grid"] == 0
    for k in ("ver_count", "ver_write", "st_count", "obj_out", "reason_out"):
        assert res[k].tolist() == res64[k].tolist()
    check(ctx, cl, objs)  # the route's own: long_min 512


@pytest.mark.parametrize("seed,width", [(11, 0), (12, 4), (13, 64)])
def test_random_batches_with_hosted_objects(ctx, seed, width):
    cl, objs = SC.random_batch(seed, 40, 300, 30, irregular_every=9)
    hosted = [SC.is_on_host(o, set(cl)) for o in objs]
    assert 0 < sum(hosted) * 8 <= len(objs)
    b, res = check(ctx, cl, objs, width)
    a = b.finish_arrays()
    assert ((a["obj_flags"] & SF.OBJ_STATUS_ON_HOST) != 0).tolist() == hosted
    for k, h in enumerate(hosted):  # the device writes 0 to a hosted object's status outputs, and still its versions
        if h:
            assert res["st_count"][k] == 0 and res["obj_out"][k] == 0 and res["reason_out"][k] == 0
    assert any(res["ver_count"][k] > 0 for k, h in enumerate(hosted) if h)
    # the device path decides the rest: the same bits as the numpy restatement
    want = SF.finish_numpy(**a)
    for k in ("ver_count", "ver_write", "st_count", "obj_out", "reason_out"):
        assert res[k].tolist() == want[k].tolist(), k


def test_last_object_ends_at_the_capacity(ctx):
    cl, objs = _NAMED["ends_at_capacity"]
    b, res = check(ctx, cl, objs, 2)
    a = b.finish_arrays()
    assert int(res["ver_count"][-1]) == int(a["ver_off"][-1] - a["ver_off"][-2]) == 4
    assert int(res["st_count"][-1]) == int(a["st_off"][-1] - a["st_off"][-2]) == 2


def test_twice_and_empty(ctx):
    from kubeadmiral_amd import runtime
    cl, objs = SC.random_batch(21, 30, 200, 20)
    b = SC.pack(cl, objs)
    first, again = finish(ctx, b), finish(ctx, b)
    a = b.finish_arrays()
    for k in ("ver_count", "ver_write", "st_count", "obj_out", "reason_out"):
        assert first[k].tobytes() == again[k].tobytes(), k
    for o in range(len(objs)):
        for off, n, keys in (("ver_off", "ver_count", ("out_ver_cluster", "out_ver_id")),
                             ("st_off", "st_count", ("out_st_cluster", "out_st_status", "out_st_gen"))):
            lo = int(a[off][o])
            for k in keys:
                assert first[k][lo:lo + first[n][o]].tobytes() == again[k][lo:lo + again[n][o]].tobytes()
    ms = ctx.sync_finish_timing()
    assert len(ms) == 3 and all(np.isfinite(m) and m >= 0 for m in ms)
    route = ctx.sync_finish_last_route()
    none = finish(ctx, SC.pack(cl, []))
    assert len(none["obj_out"]) == 0 and ctx.sync_finish_last_route() == route
    bad = b.finish_arrays()
    bad["ent_status"] = np.full_like(bad["ent_status"], 24)
    with pytest.raises(runtime.KadError) as e:
        ctx.sync_finish(*[bad.pop(k) for k in HEAD], **bad)
    assert e.value.code == runtime.KAD_EINVAL and ctx.sync_finish_last_route() == route


def rows_check(ctx, cl, objects, rows):
    b = SC.pack_rows(cl, objects, rows)
    a = b.needs_update_arrays()
    res = ctx.sync_needs_update(a.pop("n_clusters"), **a)
    assert SC.compare_rows(b, res, objects, rows) is None
    return res


def test_needs_update(ctx):
    M, st = SC.member, SC.stored
    cl = SC.names(3)
    objects = [(st([(cl[0], "gen:2"), (cl[2], "rv:7")]), "t1", "o1"), (st([(cl[0], "gen:2")], template="t0"), "t1", "o1"), (None, "t1", "o1")]
    same = M(replicas=1, surge="25%", unavailable=1, labels={"a": "b"})
    full = lambda **kw: M(2, **{**dict(replicas=1, surge="25%", unavailable=1, labels={"a": "b"}), **kw})  # noqa: E731
    rows = [(0, cl[0], same, full()),                    # recorded hit, everything equal
            (0, cl[1], same, full()),                    # recorded miss
            (1, cl[0], same, full()),                    # not current
            (2, cl[0], same, full()),                    # nothing stored
            (0, cl[2], same, M(0, "7", replicas=1, surge="25%", unavailable=1, labels={"x": "y"})),  # rv: metadata is not read
            (0, cl[0], same, full(replicas=2)), (0, cl[0], same, full(surge="30%")), (0, cl[0], same, full(unavailable=2)),
            (0, cl[0], same, full(labels={"a": "c"}))]   # each flag cleared in turn
    rows = [(o, c, d, m) for o, c, d, m in rows]
    # one row per (object, cluster) in a batch: the repeated ones go in batches of their own
    res = rows_check(ctx, cl, objects, rows[:5])
    assert res["needs_update"].tolist() == [0, 1, 1, 1, 0] and (res["recorded"] != 0).tolist() == [True, False, False, False, True]
    for row in rows[5:]:
        assert rows_check(ctx, cl, objects, [row])["needs_update"].tolist() == [1]
    r = ctx.sync_needs_update_last_route()
    assert r == {"threads": 256, "grid": 1, "stride": 256}
    assert len(ctx.sync_needs_update_timing()) == 3


@pytest.mark.parametrize("seed,C,n,per", [(1, 1, 5, 1), (2, 65, 700, 9), (3, 16384, 40, 300)])
def test_needs_update_random(ctx, seed, C, n, per):
    cl, objects, rows = SC.update_rows(seed, C, n, per)
    res = rows_check(ctx, cl, objects, rows)
    assert C == 1 or 0 < int(res["needs_update"].sum()) < len(rows)
    assert ctx.sync_needs_update_last_route()["grid"] == (len(rows) + 255) // 256


def test_schedule_results_are_left_alone(ctx):
    """A schedule's resident results read the same before and after both calls, and a later schedule repeats them."""
    import follower_cases as FC
    snap, fwk, batch, *_ = FC.resident_case()
    ctx.upload_snapshot(snap)
    ctx.upload_batch(batch)
    ctx.schedule(fwk)
    ctx.sync()
    before = ctx.download()
    cl, objs = SC.random_batch(31, 12, 50, 9)
    check(ctx, cl, objs)
    cl2, objects, rows = SC.update_rows(5, 12, 20, 4)
    rows_check(ctx, cl2, objects, rows)
    after = ctx.download()
    ctx.schedule(fwk)
    ctx.sync()
    later = ctx.download()
    for k in ("status", "count", "flags", "cluster", "replicas"):
        assert getattr(before, k).tobytes() == getattr(after, k).tobytes() == getattr(later, k).tobytes(), k


def test_group_member(ctx):
    from kubeadmiral_amd import runtime
    cl, objs = SC.random_batch(41, 20, 60, 12)
    cl2, objects, rows = SC.update_rows(6, 20, 30, 4)
    g = runtime.GroupContext([0, 0])
    try:
        check(g.member(1), cl, objs)
        rows_check(g.member(1), cl2, objects, rows)
    finally:
        g.close()


def test_end_to_end_through_the_reconciler(ctx):
    """reconcile_dispatch → reconcile_sync_versions → the operations (played here) → reconcile_sync_finish, twice over
    the same objects: the first pass creates and updates, the second finds every member current; versions, statuses
    and both write decisions against syncfin_ref at each pass."""
    import copy
    from kubeadmiral_amd import dispatch as DI
    from kubeadmiral_amd import objects as O
    from kubeadmiral_amd.controller import BatchReconciler
    names = ["m-b", "m-a", "m-d", "m-c"]  # joined in no order: the ids follow the names
    fin = DI.cascading_delete_finalizer("deployments.apps")
    clusters = [{"metadata": {"name": n, "finalizers": [fin]},
                 "status": {"conditions": [{"type": "Ready", "status": "Unknown" if n == "m-d" else "True"}]}} for n in names]
    ftc = O.FederatedTypeConfig("apps", "v1", "Deployment", "deployments", "Namespaced", "spec.replicas", "status.replicas",
                                "status.readyReplicas", "status.availableReplicas", False)
    rec = BatchReconciler(ftc, ctx=ctx)
    versions = SF.PropagatedVersions("Deployment")
    fed_ns = {"default": {"metadata": {"name": "default"}, "spec": {"placements": [
        {"controller": "kubeadmiral.io/nsautoprop-controller", "placement": {"clusters": [{"name": n} for n in names]}}]}}}

    def fed(name, placed):
        return {"metadata": {"name": name, "namespace": "default", "generation": 2, "annotations": {}},
                "spec": {"template": {}, "placements": [{"controller": "x", "placement": {"clusters": [{"name": n} for n in placed]}}]}}

    feds = [fed("web", ["m-a", "m-b", "m-d"]), fed("db", ["m-c"]), fed("none", [])]
    desired = SC.member(replicas=1, labels={"a": "b"})
    held = [{"m-a": SC.member(3, replicas=1, labels={"a": "b"}), "m-c": SC.member(4, replicas=2, labels={"a": "b"})},
            {"m-c": SC.member(0, "9", replicas=1, labels={"a": "b"})}, {}]
    tv, ov = ["t1"] * 3, ["o1"] * 3
    writes = []
    for _pass in range(2):
        out = rec.reconcile_dispatch(feds, fed_ns, clusters, held, finalizer=fin)
        want_desired = [{n: desired for n in names}] * 3
        need = rec.reconcile_sync_versions(feds, out, want_desired, names, versions, tv, ov)
        ops, ref_objs = [], []
        for k, (o, look) in enumerate(zip(out, held)):
            stored = copy.deepcopy(versions.status("default", feds[k]["metadata"]["name"]))
            recorded = R.version_get(stored, "t1", "o1")
            res = {}
            for n, op in o.ops.items():
                if op == DI.OP_CREATE:
                    look[n] = SC.member(1, replicas=1, labels={"a": "b"})
                    res[n] = {"version": "gen:1", "updated": False}
                elif op == DI.OP_UPDATE:
                    want = R.needs_update(desired, look[n], recorded.get(n, ""), "spec.replicas")
                    assert need[k][n] == (want, recorded.get(n, "")), (k, n)
                    if want:
                        g = look[n]["metadata"].get("generation", 0)
                        look[n] = SC.member(g + 1 if g else 0, "10", replicas=1, labels={"a": "b"})
                        res[n] = {"version": R.object_version(look[n]), "updated": True}
                    else:
                        res[n] = {"version": recorded[n]}
                elif op == DI.OP_DELETE:
                    del look[n]
            ops.append(res)
            records = {n: (res.get(n, {}).get("status") or s, res.get(n, {}).get("version", "")) for n, s in o.status.items()}
            ref_objs.append(SC.obj(records, sorted(o.selected), copy.deepcopy(feds[k].get("status")), stored, generation=2,
                                   resources_updated=any(r.get("updated") for r in res.values())))
        got = rec.reconcile_sync_finish(feds, out, ops, names, versions, tv, ov, now=R.NOW)
        for k, (g, o) in enumerate(zip(got, ref_objs)):
            want = R.finish(o)
            assert (g.version_status, g.version_write, g.status_write, g.reason) == \
                (want["version_status"], want["version_write"], want["status_write"], want["reason"]), (_pass, k)
            if want["status_write"]:
                assert feds[k]["status"] == want["status"]
            if want["version_write"]:
                assert versions.status("default", feds[k]["metadata"]["name"]) == want["version_status"]
        writes.append([(g.version_write, g.status_write) for g in got])
    assert feds[0]["status"]["clusters"] == [{"name": "m-a", "status": "OK", "generation": 4}, {"name": "m-b", "status": "OK", "generation": 1},
                                             {"name": "m-d", "status": "ClusterNotReady"}]
    assert feds[0]["status"]["conditions"][0]["reason"] == "CheckClusters"
    assert writes[0] == [(True, True)] * 3 and writes[1][1] == (False, False) and writes[1][2] == (False, False)
    assert writes[1][0] == (False, True)  # a ClusterNotReady cluster has no generation: clustersDiffers every time
