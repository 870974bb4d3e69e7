"""kad_deletion_plan / kad_deletion_finish on an MI355X == deletion_ref.py, the per-object restatement of the
reference's control flow, exactly: every output of both calls, and the canary bytes behind every output.

The truth table as one batch; cluster counts around the 16-byte staging loads and the LDS table's limit with the last
and with every cluster unready; objects of 0 .. C observations at every forced lane-group width and around long_min;
object counts around a block's groups and one past the grid's stride; objects that emit nothing between objects that
do; the finish call's failed operations in a group's first and last lane and on the long path, time-outs, checks absent,
NotFound, labelled, and stray rows; a schedule's results, another stage's timings and the last route untouched; a
kad_group member; a seeded gen_deletion batch against the numpy restatements; BatchReconciler end to end. Every device
call runs under a deadline of its own (``within``): a call that does not return ends the session instead of holding it."""
import concurrent.futures
import functools

import numpy as np
import pytest

import deletion_cases as DC
import deletion_ref as R
from kubeadmiral_amd import deletion as DL
from kubeadmiral_amd import synth

pytestmark = pytest.mark.gpu

WIDTHS = (1, 2, 4, 8, 16, 32, 64)
DEADLINE_S = 60
_POOL = concurrent.futures.ThreadPoolExecutor(max_workers=1)


def within(fn, *args, **kw):
    """fn(*args) with a deadline: the library call releases the interpreter lock, so a hung device shows here."""
    f = _POOL.submit(fn, *args, **kw)
    try:
        return f.result(timeout=DEADLINE_S)
    except concurrent.futures.TimeoutError:
        pytest.exit(f"a device call did not return within {DEADLINE_S} s", returncode=3)


@pytest.fixture(scope="module")
def ctx():
    from kubeadmiral_amd import build, runtime
    build.build()
    c = within(runtime.Context, 0)
    yield c
    c.close()


def run(c, arr, width=0, long_min=0):
    """Both calls on one batch, with the canaries → (plan's outputs, finish's outputs)."""
    c.deletion_debug_route(width, long_min)
    c.deletion_finish_debug_route(width, long_min)
    try:
        plan = within(c.deletion_plan, fill=DC.FILL, pad=DC.PAD, **DC.plan_args(arr))
        fin = within(c.deletion_finish, fill=DC.FILL, pad=DC.PAD, **arr)
    finally:
        c.deletion_debug_route(0, 0)
        c.deletion_finish_debug_route(0, 0)
    return plan, fin


def check(c, arr, want, width=0, long_min=0):
    plan, fin = run(c, arr, width, long_min)
    assert DC.same(plan, want, DC.PLAN_OUT, DC.PAD) is None
    assert DC.same(fin, want, DC.FINISH_OUT, DC.PAD) is None
    return plan, fin


@functools.lru_cache(maxsize=None)
def case(kind, *args):
    """(arrays, the reference's answers), computed once per case and shared."""
    if kind == "truth":
        worlds, clusters = DC.truth_batches()[args[0]]
        clusters2 = None
    elif kind == "clusters":
        C, variant = args
        n = 24 if C > 1000 else 40
        worlds, _ = DC.random_worlds(C, n, C, max_members=min(C, 6))
        names = DC.cluster_names(C)
        worlds.append(DC.world("delete", {names[C - 1]: DC.OBSERVATIONS["exists"]}, checks={names[C - 1]: "labelled"}, k=n))
        worlds.append(DC.world("delete", {}, checks={names[C - 1]: "labelled"}, k=n + 1))
        worlds.append(DC.world("orphan_all", {names[0]: DC.OBSERVATIONS["adopted"], names[C - 1]: DC.OBSERVATIONS["exists"]}, k=n + 2))
        ready = np.ones(C, bool)
        if variant == "last":
            ready[C - 1] = False
        elif variant == "all":
            ready[:] = False
        clusters = clusters2 = DC.clusters_of(ready)
        if variant == "second":  # ready at the walk, the last one unready at the checks
            ready2 = ready.copy()
            ready2[C - 1] = False
            clusters2 = DC.clusters_of(ready2)
    elif kind == "sizes":
        C, sizes = args
        worlds, clusters = DC.random_worlds(77, len(sizes), C, sizes=sizes)
        clusters2 = None
    elif kind == "tiny":
        (n,) = args
        worlds, clusters = DC.random_worlds(n, n, 3, max_members=2)
        clusters2 = None
    else:
        raise KeyError(kind)
    return DC.pack(worlds, clusters, clusters2), DC.want_of(worlds, clusters, clusters2)[0]


def test_truth_table(ctx):
    arr, want = case("truth", 0)
    plan, fin = check(ctx, arr, want)
    assert set(plan["out_op"][:len(want["out_op"])].tolist()) == {0, 3, 4}
    assert set(plan["obj_first"][:100].tolist()) == {0, 3, 4} and set(plan["obj_pre"][:100].tolist()) == {0, 2, 3}
    assert set(fin["obj_reason"][:100].tolist()) == {0, 2, 3}  # c1 is unready: no walking object gets further
    arr, want = case("truth", 1)
    plan, fin = check(ctx, arr, want)
    assert set(fin["obj_reason"][:100].tolist()) == {0, 2, 5} and set(fin["obj_status"][:100].tolist()) == {0, 1, 2}
    assert set(fin["obj_then"][:100].tolist()) == {0, 8}


CS = (1, 31, 32, 33, 64, 65, 1000, 16384)


@pytest.mark.parametrize("variant", ["ready", "last", "all", "second"])
@pytest.mark.parametrize("C", CS)
def test_cluster_counts(ctx, C, variant):
    arr, want = case("clusters", C, variant)
    plan, fin = check(ctx, arr, want)
    assert ctx.deletion_last_route()["lds"] == ctx.deletion_finish_last_route()["lds"] == (C + 15) // 16 * 16
    n = len(want["n_ops"])
    if variant == "all":
        assert not plan["n_ops"][:n].any() and not plan["n_remaining"][:n].any()
    if variant == "second":
        assert fin["obj_reason"][n - 2] == 7  # CheckNotReady wins over the failed check on the unready cluster


def _sizes(C, long_min):
    s = {0, 1, 64, 65, long_min, long_min + 1, C}
    for w in WIDTHS:
        s |= {max(w - 1, 0), w, w + 1}
    return tuple(sorted(s))


@pytest.mark.parametrize("width", WIDTHS)
def test_observations_per_object_at_every_forced_width(ctx, width):
    from kubeadmiral_amd import runtime
    long_min = runtime.deletion_route_eval(0, 0, 0, 0)["long_min"]
    C = long_min + 44
    arr, want = case("sizes", C, _sizes(C, long_min))
    assert set(np.diff(arr["obj_ob_off"]).tolist()) == set(_sizes(C, long_min))
    check(ctx, arr, want, width)
    for r in (ctx.deletion_last_route(), ctx.deletion_finish_last_route()):
        assert r["width"] == width and r["long_min"] == long_min and r["long_grid"] == 1 and r["grid"] > 0
    assert ctx.deletion_last_route()["long_grid"] == 1  # long_min + 1 and C observations: two objects, one block
    if width == 4:  # the long path's boundary moved into the short sizes, and switched off
        check(ctx, arr, want, width, long_min=7)
        assert ctx.deletion_last_route()["long_grid"] > 2
        check(ctx, arr, want, width, long_min=1 << 20)
        assert ctx.deletion_last_route()["long_grid"] == 0
        check(ctx, arr, want, 0, 0)  # the route's own width


def test_every_object_long(ctx):
    arr, want = case("sizes", 40, (9, 12, 33, 40, 21))
    check(ctx, arr, want, long_min=1)
    r = ctx.deletion_last_route()
    assert r["grid"] == 0 and r["long_grid"] == 2


@pytest.mark.parametrize("n", [1, 255, 256, 257])
def test_object_counts_around_a_block_of_one_lane_groups(ctx, n):
    arr, want = case("tiny", n)
    check(ctx, arr, want, width=1)
    assert ctx.deletion_last_route()["grid"] == (n + 255) // 256


@pytest.mark.parametrize("n", [3, 4, 5])
def test_object_counts_around_a_block_of_whole_wave_groups(ctx, n):
    arr, want = case("tiny", n)
    check(ctx, arr, want, width=64)
    assert ctx.deletion_finish_last_route()["grid"] == (n + 3) // 4


def test_every_group_takes_a_second_object(ctx):
    """One object more than the grid's stride at 32 lanes an object: the first group wraps once. The grid is read from
    the route of a batch that fills the device and is the one kad_deletion_route_eval gives for its compute units."""
    from kubeadmiral_amd import runtime
    arr, want = case("tiny", 20000)
    check(ctx, arr, want, width=32)
    grid = ctx.deletion_last_route()["grid"]
    assert grid % 8 == 0 and grid < 20000 // 8  # the resident blocks, not the objects, bound it
    n = 8 * grid + 1
    arr, want = case("tiny", n)
    check(ctx, arr, want, width=32)
    r = ctx.deletion_last_route()
    assert r["grid"] == grid and r["stride"] == n - 1
    assert runtime.deletion_route_eval(3, 1 << 22, 0, 1 << 22, grid // 8)["grid"] == grid
    assert r == ctx.deletion_finish_last_route()


def test_objects_that_emit_nothing_between_objects_that_do(ctx):
    ex = DC.OBSERVATIONS["exists"]
    quiet = [lambda k: DC.world("nothing", {"c00001": ex, "c00002": ex}, k=k), lambda k: DC.world("delete", {}, k=k),
             lambda k: DC.world("possible_orphan", {}, k=k), lambda k: DC.world("nothing", {}, k=k)]
    loud = lambda k: DC.world("delete", {"c00000": ex, "c00003": DC.OBSERVATIONS["adopted"]}, op_ok={"c00003": False}, k=k)  # noqa: E731
    worlds = []
    for pattern in ("q", "l", "qq", "l", "qqqqq", "l", "l", "q" * 70, "l", "q"):
        for ch in pattern:
            k = len(worlds)
            worlds.append(loud(k) if ch == "l" else quiet[k % 4](k))
    clusters = DC.clusters_of([True] * 5)
    arr, want = DC.pack(worlds, clusters), DC.want_of(worlds, clusters)[0]
    for width in (0, 1, 8, 64):
        plan, _ = check(ctx, arr, want, width)
    assert int((plan["n_ops"][:len(worlds)] > 0).sum()) == 5


def _finish_case(worlds, C=70, clusters2=None):
    clusters = DC.clusters_of([True] * C)
    return DC.pack(worlds, clusters, clusters2), DC.want_of(worlds, clusters, clusters2)[0]


def test_finish_failed_operations_by_lane(ctx):
    names = DC.cluster_names(300)
    ex = DC.OBSERVATIONS["exists"]
    worlds = []
    for n, bad in ((8, None), (8, 0), (8, 7), (16, 8), (16, 15), (9, 8), (300, 0), (300, 299), (300, 257)):
        members = {names[i]: ex for i in range(n)}
        worlds.append(DC.world("delete" if len(worlds) % 2 else "orphan_all", members, {} if bad is None else {names[bad]: False}, k=len(worlds)))
    arr, want = _finish_case(worlds, 300)
    assert want["n_failed_ops"].tolist() == [0] + [1] * 8
    for width in (0, 8, 16, 64):
        _, fin = check(ctx, arr, want, width)
    assert ctx.deletion_finish_last_route()["long_grid"] == 1  # the three objects of 300 observations
    assert fin["obj_reason"][:9].tolist() == [0] + [4] * 8


def test_finish_time_outs_checks_and_stray_rows(ctx):
    names = DC.cluster_names(70)
    ex = DC.OBSERVATIONS["exists"]
    every = {n: "unlabelled" for n in names}
    worlds = [
        DC.world("delete", {names[3]: ex}, wait=True),                                     # timed out
        DC.world("delete", {}, wait=True),                                                 # nothing to wait for: verified clean
        DC.world("delete", {}),                                                            # checks absent: all NotFound
        DC.world("delete", {}, checks=every),                                              # every cluster answers: unlabelled
        DC.world("delete", {}, checks=dict(every, **{names[69]: "labelled"})),             # one labelled, last
        DC.world("delete", {}, checks={names[69]: "labelled"}),
        DC.world("delete", {names[5]: ex}, checks={names[1]: "labelled", names[69]: "get_failed"}),  # remaining: stray rows
        DC.world("orphan_all", {}, checks={names[2]: "labelled"}, check_wait=True),        # not the delete arm: stray rows
        DC.world("nothing", {names[5]: ex}, checks={names[2]: "deleting"}, wait=True, check_wait=True),
        DC.world("delete", {}, check_wait=True, checks={names[0]: "deleting"}),            # the checks time out
        DC.world("possible_orphan", {names[5]: DC.OBSERVATIONS["deleting"]}, wait=True),   # no operation started
    ]
    worlds = [dict(w, fed=w["fed"] and dict(w["fed"], key=f"ns/f{k}")) for k, w in enumerate(worlds)]
    arr, want = _finish_case(worlds)
    assert want["obj_reason"].tolist() == [1, 0, 0, 0, 8, 8, 5, 0, 0, 6, 0]
    assert want["obj_then"].tolist() == [8, 3, 3, 3, 8, 8, 0, 0, 0, 8, 0]
    assert want["n_failed_checks"].tolist() == [0, 0, 0, 0, 1, 1, 0, 0, 0, 1, 0]
    for width in (0, 1, 4, 64):
        check(ctx, arr, want, width)
    check(ctx, arr, want, 0, long_min=69)  # the objects with 70 check rows alone on the long path
    assert ctx.deletion_finish_last_route()["long_grid"] == 1 and ctx.deletion_last_route()["long_grid"] == 0


def test_reason_precedence_on_the_device(ctx):
    """One object per pair of adjacent reasons with both conditions true: the earlier reason wins where the device
    computes it (del_finish_obj), at the route's own width and with one lane and a whole wave an object."""
    for worlds, clusters, clusters2, reasons in DC.precedence_worlds():
        arr, (want, traces) = DC.pack(worlds, clusters, clusters2), DC.want_of(worlds, clusters, clusters2)
        assert [t.reason for _, t in traces] == reasons
        for width in (0, 1, 64):
            _, fin = check(ctx, arr, want, width)
            assert [DC.REASONS[r] for r in fin["obj_reason"][:len(worlds)]] == reasons


def test_schedule_results_are_left_alone(ctx):
    """A schedule's resident results read the same before and after both calls, and a later schedule repeats them."""
    import follower_cases as FC
    snap, fwk, batch, *_ = FC.resident_case()
    ctx.upload_snapshot(snap)
    ctx.upload_batch(batch)
    ctx.schedule(fwk)
    ctx.sync()
    before = ctx.download()
    arr, want = case("clusters", 65, "last")
    check(ctx, arr, want)
    after = ctx.download()
    ctx.schedule(fwk)
    ctx.sync()
    later = ctx.download()
    for k in ("status", "count", "flags", "cluster", "replicas"):
        assert getattr(before, k).tobytes() == getattr(after, k).tobytes() == getattr(later, k).tobytes(), k


def test_another_stage_keeps_its_timings(ctx):
    """kad_dispatch_timing reads the same events before and after both calls; the calls' own intervals are there."""
    import dispatch_cases as DPC
    darr, _ = DPC.case("random", 5, 257, 3)
    within(ctx.dispatch_plan, **darr)
    ms = ctx.dispatch_timing()
    print("dispatch_timing read twice before the calls:", ms, ctx.dispatch_timing())
    arr, want = case("clusters", 65, "last")
    check(ctx, arr, want)
    timings = ctx.deletion_timing(), ctx.deletion_finish_timing(), ctx.dispatch_timing()
    print("deletion_timing, deletion_finish_timing, dispatch_timing after the calls:", *timings)
    for t in timings[:2]:
        assert len(t) == 3 and all(np.isfinite(m) and m >= 0 for m in t)
    assert timings[2] == ms


def test_last_route_stays_without_objects_and_after_a_rejected_batch(ctx):
    from kubeadmiral_amd import runtime
    arr, want = case("clusters", 65, "last")
    check(ctx, arr, want)
    routes = ctx.deletion_last_route(), ctx.deletion_finish_last_route()
    none = DC.pack([], DC.clusters_of([True] * 3))
    plan, fin = run(ctx, none)
    assert all((v.view(np.uint8) == DC.FILL).all() and len(v) == DC.PAD for v in list(plan.values()) + list(fin.values()))
    bad = dict(arr, ob_flags=np.full_like(arr["ob_flags"], 9))
    for call, a in ((ctx.deletion_plan, DC.plan_args(bad)), (ctx.deletion_finish, bad), (ctx.deletion_finish, dict(arr, op_ok=arr["op_ok"] + 2))):
        with pytest.raises(runtime.KadError) as e:
            within(call, **a)
        assert e.value.code == runtime.KAD_EINVAL
    assert (ctx.deletion_last_route(), ctx.deletion_finish_last_route()) == routes
    check(ctx, arr, want)  # and the calls still answer after a rejected batch


def test_before_the_first_call():
    from kubeadmiral_amd import runtime
    c = within(runtime.Context, 0)
    try:
        for f in (c.deletion_timing, c.deletion_finish_timing, c.deletion_last_route, c.deletion_finish_last_route):
            with pytest.raises(runtime.KadError) as e:
                f()
            assert e.value.code == runtime.KAD_ESTATE
        for f in (c.deletion_debug_route, c.deletion_finish_debug_route):
            with pytest.raises(runtime.KadError):
                f(3, 0)
    finally:
        c.close()


def test_group_member(ctx):
    from kubeadmiral_amd import runtime
    arr, want = case("clusters", 65, "last")
    g = runtime.GroupContext([0, 0])
    try:
        check(g.member(1), arr, want)
    finally:
        g.close()


@pytest.mark.parametrize("healthy", [1.0, 0.995])
def test_seeded_gen_deletion_batch(ctx, healthy):
    arr = synth.gen_deletion(21, 4000, 1000, healthy=healthy)
    plan, fin = run(ctx, arr)
    assert DC.same(plan, DL.plan_numpy(**DC.plan_args(arr)), DC.PLAN_OUT, DC.PAD) is None
    assert DC.same(fin, DL.finish_numpy(**arr), DC.FINISH_OUT, DC.PAD) is None
    assert ctx.deletion_last_route()["width"] == 2 and ctx.deletion_finish_last_route()["width"] == 4
    objects = list(range(0, 4000, 20))
    clusters = list(zip(DC.cluster_names(1000), (arr["cluster_flags"] & 1).astype(bool).tolist()))
    clusters2 = list(zip(DC.cluster_names(1000), (arr["chk_cluster_flags"] & 1).astype(bool).tolist()))
    want, _ = DC.want_of(DC.worlds_of_arrays(arr, objects), clusters, clusters2)
    for k in DC.PLAN_OUT[1:]:
        assert plan[k][objects].tolist() == want[k].tolist(), k
    for k in DC.FINISH_OUT:
        assert fin[k][objects].tolist() == want[k].tolist(), k
    ops = np.concatenate([plan["out_op"][arr["obj_ob_off"][o]:arr["obj_ob_off"][o + 1]] for o in objects])
    assert ops.tolist() == want["out_op"].tolist()
    if healthy == 1.0:
        assert set(fin["obj_reason"][:4000].tolist()) >= {0, 1, 2, 4, 5, 6, 8}


def test_reconciler_end_to_end(ctx):
    """A mixed batch: the live objects through reconcile_dispatch with the outcomes they have alone, the terminating
    ones (and a target without a federated object) through reconcile_deletion / reconcile_deletion_finish with the
    reference's plans and outcomes."""
    from kubeadmiral_amd import dispatch as DI
    from kubeadmiral_amd import objects as O
    from kubeadmiral_amd.controller import BatchReconciler
    ftc = O.FederatedTypeConfig("apps", "v1", "Deployment", "deployments")
    rec = BatchReconciler(ftc, ctx=ctx)
    fin_name = DI.cascading_delete_finalizer("deployments.apps")
    clusters = [{"metadata": {"name": n, "finalizers": [fin_name]}, "status": {"conditions": [{"type": "Ready", "status": "True"}]}} for n in "abcd"]

    def live(name, placed):
        return {"kind": "FederatedDeployment", "metadata": {"name": name, "namespace": "ns", "finalizers": [DL.FINALIZER_SYNC_CONTROLLER]},
                "spec": {"placements": [{"controller": "kubeadmiral.io/global-scheduler", "placement": {"clusters": [{"name": n} for n in placed]}}]}}

    err = RuntimeError("boom")
    feds = [live("l1", "ab"), DC.fed_obj("t1"), live("l2", "d"), DC.fed_obj("t2", orphan="adopted"), None, DC.fed_obj("t3"), DC.fed_obj("t4", orphan="all"),
            DC.fed_obj("t5", finalizer=False)]
    members = [{"a": DC.member_obj()}, {"a": DC.member_obj(), "c": DC.member_obj(deleting=True)}, {"c": DC.member_obj(), "d": DC.member_obj()},
               {"b": DC.member_obj(adopted=True), "d": DC.member_obj()}, {"a": DC.member_obj(), "b": err}, {}, {"c": DC.member_obj()}, {"a": DC.member_obj()}]
    terminating = [i for i, f in enumerate(feds) if f is None or "deletionTimestamp" in f["metadata"]]
    alive = [i for i in range(len(feds)) if i not in terminating]
    assert alive == [0, 2]
    fed_ns = {"ns": {"metadata": {"name": "ns"}, "spec": live("ns", "abcd")["spec"]}}
    out = within(rec.reconcile_dispatch, [feds[i] for i in alive], fed_ns, clusters, [members[i] for i in alive])
    for i, o in zip(alive, out):
        alone = within(rec.reconcile_dispatch, [feds[i]], fed_ns, clusters, [members[i]])[0]
        assert (o.selected, o.ops, o.status, o.recheck, o.reason) == (alone.selected, alone.ops, alone.status, alone.recheck, alone.reason)
    assert out[0].ops == {"a": DI.OP_UPDATE, "b": DI.OP_CREATE} and out[1].ops == {"c": DI.OP_DELETE, "d": DI.OP_UPDATE}
    t_feds, t_members = [feds[i] for i in terminating], [members[i] for i in terminating]
    plans = within(rec.reconcile_deletion, t_feds, clusters, t_members)
    op_results = [{}, {"d": False}, {}, {}, {}, {}]
    checks = [{}, {}, {}, {"b": DC.member_obj()}, {}, {}]
    outcomes = within(rec.reconcile_deletion_finish, t_feds, clusters, t_members, op_results, None, checks)
    given = within(rec.reconcile_deletion_finish, t_feds, clusters, t_members, op_results, None, checks, plans=plans)
    assert [(o.result, o.reason, o.error, o.recorded_error, o.then) for o in given] == [(o.result, o.reason, o.error, o.recorded_error, o.then) for o in outcomes]
    ref_clusters = [(n, True) for n in "abcd"]
    for fed, ms, ops, chk, p, o in zip(t_feds, t_members, op_results, checks, plans, outcomes):
        w = DC.world_of_objects(fed, ms)
        w["op_ok"] = ops
        w["checks"] = {n: "labelled" for n in chk}
        result, t = R.reconcile(w, ref_clusters)
        assert list(p.ops.items()) == [(n, {R.DELETE: DI.OP_DELETE, R.REMOVE_LABEL: DI.OP_REMOVE_LABEL}[op]) for n, op in t.ops]
        assert (p.remaining, p.retrieval_failed, p.unready) == (t.remaining, t.retrieval_failed, t.unready)
        at = t.actions.index("ops") if "ops" in t.actions else len(t.actions)
        assert (p.first, o.then) == (t.actions[:at], t.actions[at + 1:])
        assert (o.result, o.reason, o.error, o.recorded_error) == (result, t.reason, t.error, t.recorded_error)
    assert [o.result for o in outcomes] == ["Recheck", "Error", "Error", "Error", "OK", "OK"]
    assert outcomes[3].recorded_error == ('failed to delete FederatedDeployment "ns/t3": failed to verify that managed resources no longer '
                                          'exist in any cluster: one or more checks failed')
    assert within(rec.reconcile_deletion, [], clusters, []) == []
