"""kad_rollout_plan on an MI355X == the object-by-object checker (rollout_ref.py), exactly: every output is an
integer or a flag.

The golden cases of the reference in one batch; shapes (rollout_cases.py): objects with 0, 1, W - 1, W and W + 1
targets for every group width W in 1..64, 63 / 64 / 65, long_min - 1 / + 0 / + 1 and 3 * 256 + 5 targets (long_min
read from the route), every width forced, the long path forced on short objects, the serial walk forced on all; O of
1, 63, 64 and 65; named objects for each status and each pass, a budget that reaches zero at a chunk boundary and one
negative from the start; objects that may wrap int32 and ERROR objects between live ones; a seeded random batch; the
staging buffer growing, reused and shrinking; a kad_group member; reconcile_rollout end to end against the
per-object host path."""
import numpy as np
import pytest

import rollout_cases as RC
import rollout_ref as R
from kubeadmiral_amd import rollout as RO
from kubeadmiral_amd import synth

pytestmark = pytest.mark.gpu


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
    return runtime.rollout_route_eval(1, 0, 1)["long_min"]


_shapes = []


def shapes(long_min):
    if not _shapes:
        arr, marks = RC.shapes_case(long_min)
        _shapes.append((arr, marks, R.run(**arr)))
    return _shapes[0]


def assert_equal(got, want):
    assert set(got) == set(want)
    for k in want:
        g, w = np.asarray(got[k]).astype(np.int64), np.asarray(want[k], np.int64)
        assert g.shape == w.shape and (g == w).all(), (k, np.argwhere(g != w)[:5].tolist())


def test_golden_cases_in_one_batch(ctx):
    cases = RC.golden()
    arr = RC.pack([RC.from_golden(c) for c in cases])
    got = ctx.rollout_plan(**arr)
    off = arr["obj_tgt_off"]
    for k, c in enumerate(cases):
        names = sorted((t["name"] for t in c["targets"]), key=lambda s: s.encode())
        assert RO.plans_of(got, int(off[k]), int(off[k + 1]), names) == c["plans"], (c["func"], c["name"])
    assert_equal(got, R.run(**arr))
    assert ctx.rollout_last_route()["serial"] == 0


def test_staging_buffer_grows_is_reused_and_shrinks(long_min):
    from kubeadmiral_amd import runtime
    c = runtime.Context(0)
    try:
        for f in (c.rollout_timing, c.rollout_last_route):
            with pytest.raises(runtime.KadError) as e:
                f()
            assert e.value.code == runtime.KAD_ESTATE
        tiny = RC.batch([0, 2, 1], seed=5)
        want = R.run(**tiny)
        first = c.rollout_plan(**tiny)
        assert_equal(first, want)
        ms = c.rollout_timing()
        assert len(ms) == 1 and np.isfinite(ms[0]) and ms[0] >= 0
        arr, _, big_want = shapes(long_min)
        assert len(arr["tgt_flags"]) >= 100 * len(tiny["tgt_flags"])
        assert_equal(c.rollout_plan(**arr), big_want)
        again = c.rollout_plan(**tiny)
        assert_equal(again, want)
        for k in first:
            assert np.asarray(again[k]).tobytes() == np.asarray(first[k]).tobytes(), k
        # no objects: nothing launches, the last route stays
        route = c.rollout_last_route()
        assert all(len(v) == 0 for v in c.rollout_plan(**RC.pack([])).values())
        assert c.rollout_last_route() == route
    finally:
        c.close()


@pytest.mark.parametrize("width", [0] + list(RC.WIDTHS))
def test_shapes_parity_every_width(ctx, long_min, width):
    """width 0: the route's own choice."""
    from kubeadmiral_amd import runtime
    arr, marks, want = shapes(long_min)
    ctx.rollout_debug_route(width, 0, 0)
    try:
        got = ctx.rollout_plan(**arr)
        route = ctx.rollout_last_route()
    finally:
        ctx.rollout_debug_route(0, 0, 0)
    assert_equal(got, want)
    lens = np.diff(arr["obj_tgt_off"])
    live = (arr["obj_flags"] & R.OBJ_ERROR) == 0
    n_long = int(((lens > long_min) & live).sum())
    _, nowrap = runtime.rollout_check(**arr)
    n_serial = int((live & (nowrap == 0)).sum())
    assert route["long_min"] == long_min and route["long_grid"] == (n_long + 3) // 4 and n_long >= 3
    assert route["serial"] == n_serial >= 9
    if width:
        assert route["width"] == width
    else:
        ev = runtime.rollout_route_eval(len(lens), n_long, int(lens[(lens <= long_min) & live].sum()), n_serial)
        assert (route["width"], route["long_grid"], route["threads"]) == (ev["width"], ev["long_grid"], ev["threads"])
    assert set(RC.lengths(long_min)) <= set(lens.tolist())
    # the named shapes say what they were built to say
    off, st, pf = arr["obj_tgt_off"], got["status"], got["plan_flags"]
    flags = lambda name: pf[off[marks[name]]:off[marks[name] + 1]].tolist()  # noqa: E731
    assert [int(st[marks[n]]) for n in ("ok", "scale", "invalid", "error", "error-long")] == [R.OK, R.SCALE, R.INVALID, R.ERROR, R.ERROR]
    assert flags("scale") == [R.PLANNED] * 3 and not any(flags("invalid")) and not any(flags("error-long"))
    both = R.PLANNED | R.HAS_REPLICAS | R.HAS_SURGE | R.HAS_UNAVAILABLE
    o = off[marks["pass1+4"]]
    assert pf[o] == both and got["replicas"][o] == 10 and got["max_surge"][o] == 2
    o = off[marks["pass2+5"]]
    assert pf[o] == both and got["replicas"][o] == 5 and got["action"][o] == R.UPDATE
    assert flags("pass2-only")[0] == R.PLANNED | R.HAS_REPLICAS | R.ONLY_PATCH_REPLICAS
    assert got["action"][off[marks["pass2-only"]]] == R.PATCH_REPLICAS
    assert flags("pass3")[0] == R.PLANNED | R.HAS_SURGE | R.HAS_UNAVAILABLE
    assert flags("pass4-only")[0] == R.PLANNED | R.HAS_REPLICAS and got["action"][off[marks["pass4-only"]]] == R.CREATE
    z = slice(off[marks["zero-at-64"]], off[marks["zero-at-64"] + 1])
    assert got["max_surge"][z].tolist() == [1] * 64 + [0] * 66 and st[marks["zero-at-64"]] == R.OK
    assert st[marks["negative"]] in (R.OK, R.INVALID) and st[marks["empty"]] == R.OK
    assert got["action"][off[marks["to-delete"]]:off[marks["to-delete"] + 1]].tolist()[1:] == [R.DELETE, R.DELETE]


def test_long_path_and_serial_walk_forced(ctx, long_min):
    arr, _, want = shapes(long_min)
    lens = np.diff(arr["obj_tgt_off"])
    live = (arr["obj_flags"] & R.OBJ_ERROR) == 0
    for lm in (1, 3):
        ctx.rollout_debug_route(0, lm, 0)
        try:
            got = ctx.rollout_plan(**arr)
            route = ctx.rollout_last_route()
        finally:
            ctx.rollout_debug_route(0, 0, 0)
        n_long = int(((lens > lm) & live).sum())
        assert route["long_min"] == lm and route["long_grid"] == (n_long + 3) // 4 and n_long > 20
        assert_equal(got, want)
    # the serial walk for every object is the definition the prefix-sum form is held to
    for width in (0, 1, 64):
        ctx.rollout_debug_route(width, 0, 1)
        try:
            got = ctx.rollout_plan(**arr)
            assert ctx.rollout_last_route()["serial"] == int(live.sum())
        finally:
            ctx.rollout_debug_route(0, 0, 0)
        assert_equal(got, want)


@pytest.mark.parametrize("O", [1, 63, 64, 65])
def test_object_counts(ctx, O):
    rng = np.random.default_rng(O)
    arr = RC.batch(rng.integers(0, 20, O).tolist(), seed=O)
    want = R.run(**arr)
    for width in (0, 1, 64):
        ctx.rollout_debug_route(width, 0, 0)
        try:
            assert_equal(ctx.rollout_plan(**arr), want)
        finally:
            ctx.rollout_debug_route(0, 0, 0)
    ctx.rollout_debug_route(0, 1, 0)  # every object long
    try:
        arr2 = RC.batch(rng.integers(2, 20, O).tolist(), seed=O + 100)
        assert_equal(ctx.rollout_plan(**arr2), R.run(**arr2))
        assert ctx.rollout_last_route()["grid"] == 0 and ctx.rollout_last_route()["long_grid"] == (O + 3) // 4
    finally:
        ctx.rollout_debug_route(0, 0, 0)


def test_group_member(ctx, long_min):
    from kubeadmiral_amd import runtime
    arr, _, want = shapes(long_min)
    g = runtime.GroupContext([0, 0])
    try:
        assert_equal(g.member(1).rollout_plan(**arr), want)
    finally:
        g.close()


def test_seeded_random_batch(ctx):
    """1 to 33 targets, the four template fenceposts, 60 % of the targets unchanged in size, half updated: equal to
    the checker and to the numpy restatement, and at least 80 % of the objects OK with a plan."""
    a = synth.gen_rollout(7, 600, 1, 33)
    got = ctx.rollout_plan(**a)
    assert_equal(got, R.run(**a))
    ref = RO.plan_numpy(**a)
    for k in ref:
        assert (np.asarray(got[k]) == np.asarray(ref[k])).all(), k
    planned = np.add.reduceat((got["plan_flags"] & R.PLANNED).astype(np.int64), a["obj_tgt_off"][:-1])
    assert ((got["status"] == R.OK) & (planned > 0)).mean() >= 0.8
    assert ctx.rollout_last_route()["serial"] == 0


def test_reconcile_rollout_end_to_end(ctx):
    """About 150 synthetic federated Deployments through BatchReconciler against the per-object host path: the
    objects' own parsing and the checker's plan."""
    from kubeadmiral_amd import objects as O
    from kubeadmiral_amd.controller import BatchReconciler
    names = [f"member-{i:03d}" for i in range(12)]
    a = synth.gen_rollout(11, 150, 1, 12)
    feds, members, selected = synth.rollout_objects(a, names)
    feds[3]["spec"]["retainReplicas"] = True
    del members[5][names[0]]["metadata"]["annotations"][RO.LATEST_RS_NAME]  # a host error
    members[8][names[11]] = None                                           # a ready cluster without the object
    selected[8] = set(selected[8]) | {names[11]}
    feds[8]["spec"]["overrides"][0]["clusters"].append({"clusterName": names[11], "patches": [{"path": "/spec/replicas", "value": 3.0}]})
    some = sorted(selected[9])[0]
    selected[9] = set(selected[9]) - {some}                                  # no longer selected: to delete
    ftc = O.FederatedTypeConfig("apps", "v1", "Deployment", "deployments", "Namespaced", "spec.replicas", "status.replicas",
                                "status.readyReplicas", "status.availableReplicas", True)
    out = BatchReconciler(ftc, ctx=ctx).reconcile_rollout(feds, members, selected)
    assert out[3] is None and out[5].status == RO.ST_ERROR and "Failed to register target" in out[5].error
    assert set(out[5].actions.values()) == {RO.ACT_KEEP_TEMPLATE_PATCH} and not out[5].plans
    n_ok = 0
    for k, (fed, objs, sel, o) in enumerate(zip(feds, members, selected, out)):
        if k in (3, 5):
            continue
        total = RO.total_replicas(fed, ftc, sel)
        ms, mu, rev = RO.new_planner(fed, total)
        ts = []
        for name in sorted(objs):
            gone = name not in sel
            ts.append(RO.target_info(name, objs[name], 0 if gone else RO.replicas_override_for_cluster(fed, ftc, name), rev, ftc))
        want = R.plan(total, ms, mu, ts)
        assert o.plans == want, k
        for name in objs:
            p = want.get(name)
            flags = (R.EXISTS if objs[name] is not None else 0) | (R.TO_DELETE if name not in sel else 0)
            assert o.actions[name] == R.action(flags, p), (k, name)
            assert o.overrides[name] == RO.to_overrides(p)
        n_ok += o.status == RO.ST_OK and bool(o.plans)
    assert n_ok > 100 and out[8].actions[names[11]] in (RO.ACT_CREATE, RO.ACT_NONE)
    off = BatchReconciler(O.FederatedTypeConfig("apps", "v1", "Deployment", "deployments", "Namespaced", "spec.replicas"), ctx=ctx)
    assert off.reconcile_rollout(feds, members, selected) == [None] * len(feds)
