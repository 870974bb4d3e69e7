"""kad_status_aggregate on an MI355X == the object-by-object checker (sagg_ref.py), exactly: every output is an
integer.

Shapes (sagg_cases.py), both kinds: objects with 0, 1, W - 1, W and W + 1 segments for every group width W in 1..64,
63 / 64 / 65, long_min - 1 / + 0 / + 1 and 3 * 256 + 5 segments (long_min read from the route), every width forced;
the long path forced on short objects; O of 1, 63, 64 and 65; ERROR objects (short and long) between live ones, an
object whose every member is nil, sums that wrap int32, times and generations at the edge of the domain; the
staging buffer growing, reused and shrinking; a kad_group member; reconcile_status_aggregation end to end against
the per-object host path."""
import copy

import numpy as np
import pytest

import sagg_cases as SC
import sagg_ref as R
from kubeadmiral_amd import statusagg as SA
from kubeadmiral_amd import synth

pytestmark = pytest.mark.gpu

KINDS = [R.DEPLOYMENT, R.JOB]
NOW = 1_700_000_000


@pytest.fixture(scope="module")
def ctx():
    from kubeadmiral_amd import build, runtime
    build.build()
    c = runtime.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def long_min():
    from kubeadmiral_amd import runtime
    return runtime.sagg_route_eval(1, 0, 1)["long_min"]


_cases = {}


def shapes(kind, long_min):
    if kind not in _cases:
        arr, marks = SC.shapes_case(kind, long_min)
        _cases[kind] = (arr, marks, R.run(**arr))
    return _cases[kind]


def assert_equal(got, want):
    assert set(got) == set(want)
    for k in want:
        g, w = np.asarray(got[k]).astype(np.int64), np.asarray(want[k], np.int64)
        assert g.shape == w.shape and (g == w).all(), (k, np.argwhere(g != w)[:5].tolist())


@pytest.mark.parametrize("kind", KINDS)
def test_staging_buffer_grows_is_reused_and_shrinks(kind, long_min):
    """One context: a tiny batch with empty parts (an object without segments, no long object), the shapes batch
    (far larger), the tiny one again. Each step equals the checker, the third equals the first bit for bit; the
    timer and the route report KAD_ESTATE before the first call."""
    from kubeadmiral_amd import runtime
    c = runtime.Context(0)
    try:
        for f in (c.sagg_timing, c.sagg_last_route):
            with pytest.raises(runtime.KadError) as e:
                f()
            assert e.value.code == runtime.KAD_ESTATE
        tiny = SC.batch(kind, [0, 2, 1], seed=5)
        want = R.run(**tiny)
        first = c.status_aggregate(**tiny)
        assert_equal(first, want)
        _timing_ok(c.sagg_timing())
        arr, _, big_want = shapes(kind, long_min)
        assert len(arr["seg_flags"]) >= 100 * len(tiny["seg_flags"])
        assert_equal(c.status_aggregate(**arr), big_want)
        _timing_ok(c.sagg_timing())
        again = c.status_aggregate(**tiny)
        assert_equal(again, want)
        for k in first:
            assert np.asarray(again[k]).tobytes() == np.asarray(first[k]).tobytes(), k
        # no objects: nothing launches, the last route stays
        route = c.sagg_last_route()
        empty = SC.batch(kind, [])
        assert all(len(v) == 0 for k, v in c.status_aggregate(**empty).items() if k != "sums")
        assert c.sagg_last_route() == route
    finally:
        c.close()


def _timing_ok(ms):
    assert len(ms) == 1 and all(np.isfinite(t) and t >= 0 for t in ms), ms


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("width", [0] + list(SC.WIDTHS))
def test_shapes_parity_every_width(ctx, long_min, kind, width):
    """width 0: the route's own choice."""
    arr, marks, want = shapes(kind, long_min)
    ctx.sagg_debug_route(width, 0)
    try:
        got = ctx.status_aggregate(**arr)
        route = ctx.sagg_last_route()
    finally:
        ctx.sagg_debug_route(0, 0)
    assert_equal(got, want)
    lens = np.diff(arr["obj_seg_off"])
    live = (arr["obj_flags"] & R.ERROR) == 0
    n_long = int(((lens > long_min) & live).sum())
    assert route["long_min"] == long_min and route["long_grid"] == n_long >= 2
    if width:
        assert route["width"] == width
    else:
        from kubeadmiral_amd import runtime
        ev = runtime.sagg_route_eval(len(lens), n_long, int(lens[(lens <= long_min) & live].sum()))
        assert (route["width"], route["long_grid"], route["threads"]) == (ev["width"], ev["long_grid"], ev["threads"])
    assert set(SC.lengths(long_min)) <= set(lens.tolist())
    # the named shapes say what they were built to say
    for name in ("error", "error-long"):
        o = marks[name]
        assert all(int(np.asarray(got[k])[..., o].any()) == 0 for k in got), name
    o = marks["all-nil"]
    assert not got["sums"][:, o].any()
    if kind == R.DEPLOYMENT:
        assert got["observed"][o] == arr["obj_observed"][o]
        assert got["observed"][marks["edge-times"]] == arr["obj_generation"][marks["edge-times"]]
        assert got["sums"][:, marks["wrap"]].tolist() == [-2 ** 31 + 5, 2 ** 31 - 8, -2 ** 30, 24, 24]
    else:
        assert (got["start_min"][o], got["done_max"][o], got["finished"][o]) == (R.NONE_START, R.NONE_DONE, 0)
        e = marks["edge-times"]
        assert (got["start_min"][e], got["done_max"][e], got["n_done"][e], got["finished"][e]) == (-SC.TMAX, SC.TMAX, 4, 1)
        assert got["sums"][:, marks["wrap"]].tolist() == [-2 ** 31 + 5, 2 ** 31 - 8, -2 ** 30]
    assert 0 < int(got["changed"].sum()) < int(live.sum())


@pytest.mark.parametrize("kind", KINDS)
def test_long_path_forced_on_short_objects(ctx, kind, long_min):
    arr, _, want = shapes(kind, long_min)
    for lm in (1, 3):
        ctx.sagg_debug_route(0, lm)
        try:
            got = ctx.status_aggregate(**arr)
            route = ctx.sagg_last_route()
        finally:
            ctx.sagg_debug_route(0, 0)
        lens = np.diff(arr["obj_seg_off"])
        assert route["long_min"] == lm and route["long_grid"] == int(((lens > lm) & ((arr["obj_flags"] & R.ERROR) == 0)).sum()) > 20
        assert_equal(got, want)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("O", [1, 63, 64, 65])
def test_object_counts(ctx, kind, O):
    rng = np.random.default_rng(O)
    arr = SC.batch(kind, rng.integers(0, 20, O).tolist(), seed=O)
    want = R.run(**arr)
    for width in (0, 1, 64):
        ctx.sagg_debug_route(width, 0)
        try:
            assert_equal(ctx.status_aggregate(**arr), want)
        finally:
            ctx.sagg_debug_route(0, 0)
    # every object long
    ctx.sagg_debug_route(0, 1)
    try:
        arr2 = SC.batch(kind, rng.integers(2, 20, O).tolist(), seed=O + 100)
        assert_equal(ctx.status_aggregate(**arr2), R.run(**arr2))
        assert ctx.sagg_last_route()["grid"] == 0 and ctx.sagg_last_route()["long_grid"] == O
    finally:
        ctx.sagg_debug_route(0, 0)


@pytest.mark.parametrize("kind", KINDS)
def test_group_member(ctx, kind, long_min):
    from kubeadmiral_amd import runtime
    arr, _, want = shapes(kind, long_min)
    g = runtime.GroupContext([0, 0])
    try:
        assert_equal(g.member(1).status_aggregate(**arr), want)
    finally:
        g.close()


@pytest.mark.parametrize("kind", KINDS)
def test_synthetic_batch_against_numpy_and_checker(ctx, kind):
    a, _ = synth.gen_status_aggregation(7, kind, 3000, 600, duplicate_share=0.002)
    got = ctx.status_aggregate(**a)
    assert_equal(got, R.run(**a))
    ref = SA.sagg_numpy(**a)
    for k in ref:
        assert (np.asarray(got[k]) == np.asarray(ref[k])).all(), k
    route = ctx.sagg_last_route()
    assert route["long_grid"] > 0 and route["grid"] > 0 and route["width"] == 1


def test_reconcile_status_aggregation_end_to_end(ctx):
    """About 200 synthetic objects of both kinds through BatchReconciler against the per-object host path; a
    second pass over the applied objects (same ``now``) finds nothing to update."""
    from kubeadmiral_amd.controller import STATUS_ALL_OK, STATUS_ERROR, BatchReconciler
    names = [f"member-{i:03d}" for i in range(24)]
    sources, feds, members = [], [], []
    for kind in KINDS:
        a, seg_cluster = synth.gen_status_aggregation(11, kind, 100, len(names), duplicate_share=0.03, changed=0.3)
        s, f, m = synth.status_aggregation_objects(a, seg_cluster, names)
        sources += s
        feds += f
        members += m
    # an object-level error, a deleted source and a missing federated object between live ones
    members[5] = dict(members[5], broken={"kind": "Deployment", "status": {"replicas": "three"}})
    sources[7]["metadata"]["deletionTimestamp"] = "2024-01-01T00:00:00Z"
    feds[9] = None
    host = copy.deepcopy(sources)
    want = []
    for src, fed, objs in zip(host, feds, members):
        if fed is None or "deletionTimestamp" in src["metadata"]:
            want.append((STATUS_ALL_OK, False))
            continue
        try:
            utd = SA.is_resource_propagated(src, fed)
            need = SA.aggregate_deployment(src, fed, objs, utd) if src["kind"] == "Deployment" else \
                SA.aggregate_job(src, fed, objs, utd, NOW)
            want.append((STATUS_ALL_OK, need))
        except SA.StatusAggError:
            want.append((STATUS_ERROR, False))
    from kubeadmiral_amd import objects as O
    ftc = O.FederatedTypeConfig("apps", "v1", "Deployment", "deployments", "Namespaced", "spec.replicas",
                                "status.replicas", "status.readyReplicas")
    rec = BatchReconciler(ftc, ctx=ctx)
    out = rec.reconcile_status_aggregation(sources, feds, members, now=NOW)
    assert [(o.status, o.need_update) for o in out] == want
    assert want[5] == (STATUS_ERROR, False) and out[5].error
    assert all(SA.deep_equal(a, b) for a, b in zip(sources, host))
    assert 20 < sum(n for _, n in want) and any(not n for _, n in want[100:])
    # the checker agrees on the statuses, object by object
    for src, fed, objs, (st, _) in zip(sources, feds, members, want):
        if st == STATUS_ALL_OK and fed is not None and "deletionTimestamp" not in src["metadata"]:
            if src["kind"] == "Deployment":
                new, _ = R.deployment({"metadata": src["metadata"], "status": src["status"]}, fed, objs, SA.is_resource_propagated(src, fed))
                new_obs = new.pop("observedGeneration", None), src["status"].get("observedGeneration")
                assert R.go_equal(new, {k: v for k, v in src["status"].items() if k != "observedGeneration"}), new_obs
            else:
                assert R.go_equal(R.job(src, objs, NOW)[0], src["status"])
    again = rec.reconcile_status_aggregation(sources, feds, members, now=NOW)
    assert not any(o.need_update for o in again) and [o.status for o in again] == [o.status for o in out]
