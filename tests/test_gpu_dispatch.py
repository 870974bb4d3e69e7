"""kad_dispatch_plan on an MI355X == the cluster-by-cluster checker (dispatch_ref.py), exactly: every output is an
integer.

The truth table of the decision in one batch; shapes (dispatch_cases.py) at C of 1, 31, 32, 33, 63, 64, 65, 1000 and
16384; O of 1, 3, 4, 5, 63, 64, 65 and one more than four times the grid of tiny objects; ascending order, counts
within the capacity and untouched bytes behind them in every comparison (the output arrays start as a pattern); the
staging buffer growing, reused and shrinking; a kad_group member; a seeded random batch; reconcile_dispatch end to
end against the per-object host path, and into reconcile_rollout."""
import numpy as np
import pytest

import dispatch_cases as DC
import dispatch_ref as R
from kubeadmiral_amd import dispatch as DI
from kubeadmiral_amd import synth

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from kubeadmiral_amd import build, runtime
    build.build()
    c = runtime.Context(0)
    yield c
    c.close()


def check(got, arr, want):
    """Equal to the checker, the pattern intact behind every object's entries, ascending within an object."""
    assert DC.entries_equal(got, want, arr["out_off"], DC.FILL) is None
    off, count = arr["out_off"], got["count"]
    assert (count >= 0).all() and (count <= np.diff(off)).all()
    for o in np.flatnonzero(count > 1):
        assert (np.diff(got["out_cluster"][off[o]:off[o] + count[o]]) > 0).all(), o


def test_truth_table(ctx):
    arr, want = DC.case("truth")
    got = ctx.dispatch_plan(fill=DC.FILL, **arr)
    check(got, arr, want)
    _, combos = DC.truth_table()
    off, seen = arr["out_off"], set()
    for o, (sel, ob, orphan) in enumerate(combos):
        for i in range(int(off[o]), int(off[o]) + int(got["count"][o])):
            seen.add((int(got["out_op"][i]), R.STATUSES[got["out_status"][i]]))
    assert seen == {(R.NONE, "ClusterNotReady"), (R.NONE, "CachedRetrievalFailed"), (R.NONE, "WaitingForRemoval"),
                    (R.REMOVE_LABEL, "LabelRemovalTimedOut"), (R.DELETE, "DeletionTimedOut"), (R.NONE, "ClusterTerminating"),
                    (R.NONE, "FinalizerCheckFailed"), (R.CREATE, "CreationTimedOut"), (R.UPDATE, "UpdateTimedOut")}
    # the branches that record nothing, and the recheck
    assert (got["count"] < 16).all() and (got["count"] == 0).any()
    recheck = np.array([sel and ob != R.RETRIEVAL_FAILED for sel, ob, _ in combos])  # a failed lookup comes first
    assert ((got["obj_result"] == R.RECHECK) == recheck).all()
    assert got["n_selected"].tolist() == [16 if sel else 0 for sel, _, _ in combos]


@pytest.mark.parametrize("C", DC.SHAPE_CS)
def test_shapes(ctx, C):
    arr, want = DC.case("shapes", C)
    got = ctx.dispatch_plan(fill=DC.FILL, **arr)
    check(got, arr, want)
    assert ctx.dispatch_last_route()["words"] == (C + 31) // 32
    zero = (got["count"] == 0) & (np.diff(arr["out_off"]) > 0)
    assert zero[(arr["obj_ns"] == 1) | (arr["obj_ns"] == 2)].all() and got["n_selected"].max() == C


@pytest.mark.parametrize("n", [1, 3, 4, 5, 63, 64, 65])
def test_object_counts(ctx, n):
    arr, want = DC.case("random", n, 257, 3)
    check(ctx.dispatch_plan(fill=DC.FILL, **arr), arr, want)
    assert ctx.dispatch_last_route()["grid"] == (n + 3) // 4


def test_every_wave_takes_a_second_object(ctx):
    """One more than 4 x grid one-cluster objects, the grid read from the route of a batch that fills it: a bitmap
    word left over from a wave's first object would show in its second."""
    arr, want = DC.case("tiny", 12000)
    check(ctx.dispatch_plan(fill=DC.FILL, **arr), arr, want)
    grid = ctx.dispatch_last_route()["grid"]
    assert grid < 3000  # the resident blocks, not the objects, bound it
    n = 4 * grid + 1
    arr, want = DC.case("tiny", n)
    got = ctx.dispatch_plan(fill=DC.FILL, **arr)
    route = ctx.dispatch_last_route()
    assert route["grid"] == grid and route["stride"] == 4 * grid == n - 1
    check(got, arr, want)
    assert (got["n_selected"] == 1).all() and (got["count"] <= 2).all()


def test_staging_buffer_grows_is_reused_and_shrinks():
    from kubeadmiral_amd import runtime
    c = runtime.Context(0)
    try:
        for f in (c.dispatch_timing, c.dispatch_last_route):
            with pytest.raises(runtime.KadError) as e:
                f()
            assert e.value.code == runtime.KAD_ESTATE
        tiny, want = DC.case("random", 5, 257, 3)
        first = c.dispatch_plan(fill=DC.FILL, **tiny)
        check(first, tiny, want)
        ms = c.dispatch_timing()
        assert len(ms) == 3 and all(np.isfinite(m) and m >= 0 for m in ms)
        big, big_want = DC.case("shapes", 1000)
        assert int(big["out_off"][-1]) >= 100 * int(tiny["out_off"][-1])
        check(c.dispatch_plan(fill=DC.FILL, **big), big, big_want)
        again = c.dispatch_plan(fill=DC.FILL, **tiny)
        check(again, tiny, want)
        for k in first:
            assert np.asarray(again[k]).tobytes() == np.asarray(first[k]).tobytes(), k
        # no objects: nothing launches, the last route stays
        route = c.dispatch_last_route()
        none = c.dispatch_plan(**DC.pack(DC.mixed_flags(257), []))
        assert all(len(v) == 0 for v in none.values())
        assert c.dispatch_last_route() == route
        with pytest.raises(runtime.KadError) as e:
            c.dispatch_plan(**DC.pack([DC.HEALTHY] * 16385, [DC.obj(pl=[0])]))
        assert e.value.code == runtime.KAD_EUNSUPPORTED and c.dispatch_last_route() == route
    finally:
        c.close()


def test_group_member(ctx):
    from kubeadmiral_amd import runtime
    arr, want = DC.case("shapes", 65)
    g = runtime.GroupContext([0, 0])
    try:
        check(g.member(1).dispatch_plan(fill=DC.FILL, **arr), arr, want)
    finally:
        g.close()


def test_seeded_random_batch(ctx):
    """600 objects over 257 clusters with mixed cluster flags: equal to the checker and to the numpy restatement, and
    at least 80 % of the entries are creates or updates."""
    arr, want = DC.case("synth", 9, 600, 257)
    got = ctx.dispatch_plan(fill=DC.FILL, **arr)
    check(got, arr, want)
    assert DC.entries_equal(got, DI.plan_numpy(fill=DC.FILL, **arr), arr["out_off"], DC.FILL) is None
    live = np.concatenate([np.arange(o, o + c) for o, c in zip(arr["out_off"][:-1], got["count"])]).astype(np.int64)
    assert np.isin(got["out_op"][live], (R.CREATE, R.UPDATE)).mean() >= 0.8
    assert len(set(arr["cluster_flags"].tolist())) > 4


def test_reconcile_dispatch_end_to_end(ctx):
    """About 100 synthetic federated Deployments over 12 clusters, one not ready, one terminating with cascading
    delete and one without, one without the finalizer: BatchReconciler against the checker walked per object over
    names, then its selected / rollout_members through reconcile_rollout against hand-built inputs."""
    from kubeadmiral_amd import objects as O
    from kubeadmiral_amd.controller import BatchReconciler
    names = [f"member-{i:03d}" for i in range(12)]
    fin = DI.cascading_delete_finalizer("deployments.apps")
    flags = {n: R.READY | R.FINALIZER for n in names}
    flags[names[2]] = R.FINALIZER
    flags[names[5]] = R.READY | R.FINALIZER | R.TERMINATING | R.CASCADING
    flags[names[7]] = R.READY | R.FINALIZER | R.TERMINATING
    flags[names[9]] = R.READY
    clusters = []
    for n in names:
        f = flags[n]
        meta = {"name": n, "finalizers": [fin] if f & R.FINALIZER else []}
        if f & R.TERMINATING:
            meta["deletionTimestamp"] = "2024-01-01T00:00:00Z"
        if f & R.CASCADING:
            meta["annotations"] = {DI.CASCADING_DELETE_ANNOTATION: "true"}
        clusters.append({"metadata": meta, "status": {"conditions": [{"type": "Ready", "status": "True" if f & R.READY else "Unknown"}]}})
    a = synth.gen_rollout(13, 100, 1, 12)
    feds, members, selected = synth.rollout_objects(a, names)
    rng = np.random.default_rng(5)
    lookups = []
    for k, (fed, objs, sel) in enumerate(zip(feds, members, selected)):
        placed = sorted(sel)
        if k % 7 == 0:  # the placement has moved on from a cluster that still holds the object
            placed = placed[1:] + [names[int(rng.integers(12))]]
        fed["spec"]["placements"] = [{"controller": "kubeadmiral.io/global-scheduler", "placement": {"clusters": [{"name": n} for n in placed[::-1]]}},
                                     {"controller": "other", "placement": {"clusters": [{"name": n} for n in placed[:1] + ["not-joined"]]}}]
        if k % 5 == 0:
            fed["metadata"]["annotations"][DI.ORPHAN_ANNOTATION] = ("all", "adopted")[k % 2]
        look = dict(objs)
        if k % 11 == 0:
            for n in (sorted(objs)[-1], names[5]):
                if n in look:
                    look[n]["metadata"]["deletionTimestamp"] = "2024-01-01T00:00:00Z"
        if k % 4 == 0:
            for n in (sorted(objs)[-1], names[5]):
                if n in look:
                    look[n]["metadata"]["annotations"][DI.ADOPTED_ANNOTATION] = "true"
        if k % 9 == 0:
            look[sorted(objs)[0]] = LookupError("cache not synced")
        lookups.append(look)
    feds[17]["spec"]["placements"] = "not a list"
    ftc = O.FederatedTypeConfig("apps", "v1", "Deployment", "deployments", "Namespaced", "spec.replicas", "status.replicas",
                                "status.readyReplicas", "status.availableReplicas", True)
    fed_ns = {"default": {"metadata": {"name": "default"}, "spec": {"placements": [
        {"controller": "kubeadmiral.io/nsautoprop-controller", "placement": {"clusters": [{"name": n} for n in names[:11]]}}]}}}
    rec = BatchReconciler(ftc, ctx=ctx)
    out = rec.reconcile_dispatch(feds, fed_ns, clusters, lookups)
    assert len(out) == 100 and out[17].reason == "ComputePlacementFailed" and not out[17].status and not out[17].selected
    seen = set()
    for k, (fed, look, o) in enumerate(zip(feds, lookups, out)):
        if k == 17:
            continue
        placed = [c["name"] for p in fed["spec"]["placements"] for c in p["placement"]["clusters"]]
        want_sel = R.compute_placement(placed, names, "intersect", names[:11])
        ann = fed["metadata"]["annotations"].get(DI.ORPHAN_ANNOTATION, "")
        view = {n: "error" if isinstance(m, Exception) else
                R.EXISTS | (R.DELETING if "deletionTimestamp" in m["metadata"] else 0) |
                (R.ADOPTED if m["metadata"]["annotations"].get(DI.ADOPTED_ANNOTATION) == "true" else 0) for n, m in look.items()}
        recorded, n_ops, recheck = R.sync_to_clusters([(n, flags[n]) for n in names], want_sel, view, ann)
        assert o.selected == want_sel and o.recheck == recheck and o.reason is None, k
        assert o.status == {n: s for n, _, s in recorded} and o.ops == {n: op for n, op, _ in recorded if op != R.NONE}, k
        assert o.to_delete == {n for n, op, _ in recorded if op in (R.DELETE, R.REMOVE_LABEL)}
        assert o.rollout_members == {n: look.get(n) for n in names if flags[n] & R.READY and not isinstance(look.get(n), Exception)
                                     and (n in want_sel or look.get(n) is not None)}, k
        seen |= set(o.status.values())
    assert seen == set(R.STATUSES[1:])
    # the dispatch plan's products are reconcile_rollout's inputs
    keep = [k for k in range(100) if k != 17]
    got = rec.reconcile_rollout([feds[k] for k in keep], [out[k].rollout_members for k in keep], [out[k].selected for k in keep])
    hand = rec.reconcile_rollout(
        [feds[k] for k in keep],
        [{n: lookups[k].get(n) for n in names if flags[n] & R.READY and not isinstance(lookups[k].get(n), Exception)
          and (n in out[k].selected or lookups[k].get(n) is not None)} for k in keep],
        [R.compute_placement([c["name"] for p in feds[k]["spec"]["placements"] for c in p["placement"]["clusters"]], names,
                             "intersect", names[:11]) for k in keep])
    assert len(got) == len(hand) == 99
    for g, h in zip(got, hand):
        assert (g.status, g.plans, g.overrides, g.actions, g.error) == (h.status, h.plans, h.overrides, h.actions, h.error)
    assert sum(g.status == 0 and bool(g.plans) for g in got) > 50
