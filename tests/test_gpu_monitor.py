"""kad_monitor_reconcile and kad_monitor_report on an MI355X == the per-object checker (monitor_ref.py), exactly: every
output is an integer or a flag. The harness of monitor_cases.py compares the worker result, the annotation decision,
the log line, the stored meter (read back through kad_monitor_read), the lastStatus map and the report's metrics and
timer lists (ascending slot order) after every step.

The named cases and seeded batches at every lane-group width (forced through kad_monitor_reconcile_debug_route) and on
the block path; lists of 0, 1, width - 1, width, width + 1 and 2 * width + 1 entries; one list of a few thousand entries
that differs in its last; cluster counts of 1, 64, 65 and 16384; reports at table sizes around the wave and block
tiles, with the grid forced to 1 and 2 blocks, dead slots between live ones, every threshold at its boundary and one
nanosecond past it, n_types of 1, the bins limit and limit + 1 on both histogram paths; the table's lifecycle."""
import numpy as np
import pytest

import monitor_cases as MC
import monitor_ref as R
from kubeadmiral_amd import monitor as M

pytestmark = pytest.mark.gpu

WIDTHS = (1, 2, 4, 8, 16, 32, 64)
T0, S, MIN = MC.T0, MC.S, MC.MIN
ROUTES = [(w, 0) for w in WIDTHS] + [(0, 1)]  # (width, long_min): long_min 1 sends every list of two entries to a block


@pytest.fixture(scope="module")
def ctx():
    from kubeadmiral_amd import build, runtime
    build.build()
    c = runtime.Context(0)
    yield c
    c.close()


def device(ctx, width=0, long_min=0):
    return lambda table: MC.DeviceBackend(ctx, width, long_min)


@pytest.mark.parametrize("width,long_min", ROUTES)
def test_named_cases(ctx, width, long_min):
    for name, case in MC.CASES.items():
        assert MC.run_case(case, device(ctx, width, long_min)) is None, name
    route = ctx.monitor_reconcile_last_route()
    assert route["width"] == (width or 1) and route["long_min"] == (long_min or 512)


@pytest.mark.parametrize("width,long_min", [(0, 0), (1, 0), (4, 0), (64, 0), (0, 1), (8, 3)])
def test_seeded(ctx, width, long_min):
    assert MC.run_seeded(11 + width, device(ctx, width, long_min), n_objects=60, n_clusters=9, rounds=3) is None


def interned(h, C):
    for i in range(C):
        h.table.cluster_id(f"c{i:05d}")
    return [f"c{i:05d}" for i in range(C)]


def list_events(h, names, sizes, now):
    """Per size three meters with a lastStatus of that many entries and a non-zero duration, and their events: the
    member list equal to lastStatus and not to fed; differing from lastStatus in its last entry alone; equal to fed."""
    seeds, events = [], []
    for n in sizes:
        last = {c: 1 for c in names[:n]}
        bumped = dict(last)
        if n:
            bumped[names[n - 1]] = 2
        other = bumped if n else {names[0]: 1}
        for tag, fed, mem in (("same", other, last), ("last", last, bumped if n else other), ("sync", last, last)):
            key = f"FederatedDeployment/lists/{tag}-{n}"
            seeds.append(MC.seed(last, now - 400 * S, 7 * MIN, key=key))
            events.append(MC.ev(MC.synced_obj(), MC.fed(sorted(fed.items())), MC.mem(sorted(mem.items())), key=key))
    h.seed(seeds)
    return events


@pytest.mark.parametrize("width", WIDTHS)
def test_list_lengths_around_the_width(ctx, width):
    h = MC.Harness(device(ctx, width))
    sizes = sorted({0, 1, max(0, width - 1), width, width + 1, 2 * width + 1})
    events = list_events(h, interned(h, 2 * width + 2), sizes, T0)
    assert h.step(T0, events) is None
    assert ctx.monitor_reconcile_last_route()["width"] == width
    assert h.report_diff(T0) is None


def test_long_list_differs_in_its_last_entry(ctx):
    h = MC.Harness(device(ctx))
    events = list_events(h, interned(h, 3001), [3000, 513, 512, 5], T0)
    assert h.step(T0, events) is None
    route = ctx.monitor_reconcile_last_route()
    assert route["long_grid"] == 6 and route["grid"] > 0  # 3000 and 513 on the block path, 512 and 5 on the group path


@pytest.mark.parametrize("C", [1, 64, 65, 16384])
def test_cluster_counts(ctx, C):
    h = MC.Harness(device(ctx))
    events = list_events(h, interned(h, C), [C], T0)
    assert h.step(T0, events) is None
    assert len(h.table.clusters) == C
    if C == 16384:
        from kubeadmiral_amd import runtime
        h.table.cluster_id("one-more")
        fresh = MC.ev(MC.synced_obj(), key="FederatedDeployment/lists/fresh")
        with pytest.raises(runtime.KadError) as e:
            h.table.reconcile(events[:1] + [fresh], T0, h.be.run, h.be.reserve)
        assert e.value.code == runtime.KAD_EUNSUPPORTED
        assert fresh["key"] not in h.table.slot_of and h.state_diff() is None  # the failed call's slot went back


def table_seeds(n, now, rng, kinds=("FederatedDeployment", "FederatedJob", "FederatedSecret")):
    """n meters of every report class: synced long ago, synced within the interval, late by random amounts, out of
    sync by random amounts, never status-synced, without a creation time."""
    seeds = []
    for i in range(n):
        r = rng.random()
        cr = now - int(rng.integers(1, 3 * 86400)) * S
        lu = None if rng.random() < 0.3 else cr + int(rng.integers(0, 3600)) * S
        if r < 0.35:
            ss = (lu or cr) + int(rng.integers(1, 10 ** 10))
        elif r < 0.6:
            ss = now - int(rng.integers(0, 120)) * S + int(rng.integers(0, S))
        else:
            ss = None if rng.random() < 0.3 else cr - int(rng.integers(1, 1000)) * S
        if rng.random() < 0.1:
            cr = None
        oos = 0 if rng.random() < 0.5 else int(rng.integers(1, 2 * 86400)) * S
        lst = None if rng.random() < 0.2 else now - int(rng.integers(0, 86400)) * S
        seeds.append(MC.seed({} if lst else None, lst, oos, creation=cr, lu=lu, ss=ss, key=f"{kinds[i % len(kinds)]}/t/o{i}"))
    return seeds


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025])
def test_report_table_sizes(ctx, n):
    h = MC.Harness(device(ctx))
    h.seed(table_seeds(n, T0, np.random.default_rng(n)))
    assert ctx.monitor_info()["n_slots"] == n
    assert h.report_diff(T0) is None
    route = ctx.monitor_report_last_route()
    assert route["grid"] == (n + 1023) // 1024 and route["wtiles"] == (n + 255) // 256


@pytest.mark.parametrize("grid", [1, 2, 0])
@pytest.mark.parametrize("path", [1, 2])
def test_report_stride_scan_and_dead_slots(ctx, grid, path):
    h = MC.Harness(device(ctx))
    rng = np.random.default_rng(5)
    seeds = table_seeds(5000, T0, rng)
    h.seed(seeds)
    dead = [s["key"] for s in seeds if rng.random() < 0.3]
    assert h.step(T0, [MC.ev(None, key=k) for k in dead]) is None
    ctx.monitor_report_debug_route(path, grid)
    try:
        assert h.report_diff(T0) is None
        route = ctx.monitor_report_last_route()
        assert route["grid"] == (grid or 5) and route["path"] == path - 1
        r = ctx.monitor_report(T0, h.table.n_types, timer_cap=3)  # the lists grow to their lengths
        assert len(r["sync_slot"]) == r["n_timers"][0] > 3
        assert ctx._monitor_timer_cap >= r["n_timers"].max()  # the next report starts with room for them
    finally:
        ctx.monitor_report_debug_route(0, 0)
    info = ctx.monitor_info()
    assert info["n_slots"] == 5000 and info["n_live"] == 5000 - len(dead)


def test_thresholds_at_and_past_the_boundary(ctx):
    """After and > are strict: a meter exactly at a threshold is not counted, one nanosecond past it is."""
    h = MC.Harness(device(ctx))
    seeds = []
    for b, (_, minutes) in enumerate(M.BUCKETS):
        for d in (0, 1):
            # late: the last update is after the sync success; start = now - bucket - d
            seeds.append(MC.seed({}, T0 - S, minutes * MIN + d, creation=T0 - 3 * 86400 * S, lu=T0 - minutes * MIN - d,
                                 ss=T0 - 2 * 86400 * S, key=f"FederatedJob/b/late-{b}-{d}"))
    for d in (0, 1):
        seeds.append(MC.seed({}, T0 - S, MIN + d, key=f"FederatedJob/b/status-{d}"))       # outOfSync > ReportInterval
        seeds.append(MC.seed(None, None, MIN + 1, key=f"FederatedJob/b/nosync-{d}"))      # lastStatusSynced is zero
        seeds.append(MC.seed(None, None, 0, creation=T0 - 2 * MIN, ss=T0 - MIN + d, key=f"FederatedJob/b/fresh-{d}"))
        seeds.append(MC.seed(None, None, 0, creation=T0 - 30 * S, lu=T0 - 30 * S, ss=T0 - 30 * S + d, key=f"FederatedJob/b/equal-{d}"))
    h.seed(seeds)
    assert h.report_diff(T0) is None
    r = ctx.monitor_report(T0, h.table.n_types)
    # bucket j counts the meters one nanosecond past buckets j.. and those exactly at the buckets above j
    assert r["counters"][:6].tolist() == [11, 9, 7, 5, 3, 1] and r["counters"][6:12].tolist() == [11, 9, 7, 5, 3, 1]
    assert r["counters"][12:].tolist() == [2, 13] and r["sync_ms"].tolist() == [60000, 0]


@pytest.mark.parametrize("n_types", [1, 4096, 4097])
@pytest.mark.parametrize("path", [1, 2])
def test_type_histogram_paths(ctx, n_types, path):
    from kubeadmiral_amd import runtime
    h = MC.Harness(device(ctx))
    kinds = [f"Kind{i}" for i in range(n_types)]
    for k in kinds:
        h.table.kind_id(k + "/x")
    rng = np.random.default_rng(n_types)
    pick = [kinds[0], kinds[-1]] + [kinds[int(i)] for i in rng.integers(0, n_types, 300)]
    h.seed(table_seeds(len(pick), T0, rng, kinds=pick))
    ctx.monitor_report_debug_route(path, 0)
    try:
        if path == 1 and n_types > 4096:
            with pytest.raises(runtime.KadError) as e:
                ctx.monitor_report(T0, n_types)
            assert e.value.code == runtime.KAD_EINVAL
        else:
            assert h.report_diff(T0) is None
            assert ctx.monitor_report_last_route()["path"] == path - 1
    finally:
        ctx.monitor_report_debug_route(0, 0)
    assert h.report_diff(T0) is None  # the route's own path
    assert ctx.monitor_report_last_route()["path"] == (0 if n_types <= 4096 else 1)
    with pytest.raises(runtime.KadError):
        ctx.monitor_report(T0, n_types - 1)  # a stored type id is out of range


def test_out_of_sync_leaves_the_stored_meter(ctx):
    """The reference changes its local meter on ErrStatusOutOfSync and does not store it: kad_monitor_read shows the
    status columns as monitor_load left them, the outputs carry the would-be values."""
    h = MC.Harness(device(ctx))
    h.seed(MC.CASES["out_of_sync_meter_untouched"]["seed"])
    slot = h.table.slot_of[MC.K]
    before = ctx.monitor_read([slot])
    o = h.table.reconcile([MC.CASES["out_of_sync_meter_untouched"]["steps"][0][1]], T0, h.be.run, h.be.reserve)[0]
    after = ctx.monitor_read([slot])
    assert o.result == "REQUEUE" and o.requeue_after_s == 5 and not o.status_stored
    assert (o.log_last_status_synced, o.log_out_of_sync_ns, o.log_last_status) == (T0 - 900 * S, 900 * S, dict(MC.A3))
    for k in ("last_status_synced", "out_of_sync_ns", "creation"):
        assert before[k].tolist() == after[k].tolist()
    assert after["out_of_sync_ns"].tolist() == [11 * MIN] and h.table.last[slot][1].tolist() == [2, 2]


def test_table_lifecycle(ctx):
    from kubeadmiral_amd import runtime
    h = MC.Harness(device(ctx))
    h.seed(table_seeds(300, T0, np.random.default_rng(1)))
    slots = np.arange(300, dtype=np.int32)
    before = ctx.monitor_read(slots)
    cap = ctx.monitor_info()["capacity"]
    ctx.monitor_reserve(cap + 5000)  # growth keeps the contents
    assert ctx.monitor_info()["capacity"] >= cap + 5000
    after = ctx.monitor_read(slots)
    for k in before:
        assert before[k].tobytes() == after[k].tobytes(), k
    assert h.report_diff(T0) is None and h.state_diff() is None
    with pytest.raises(runtime.KadError) as e:
        ctx.monitor_read([ctx.monitor_info()["capacity"]])
    assert e.value.code == runtime.KAD_ENOSPC
    with pytest.raises(runtime.KadError):
        ctx.monitor_read([3, 3])
    # the same batch twice: the second call finds the meters the first left
    events = [MC.ev(MC.synced_obj(), MC.fed(MC.A2), MC.mem(MC.A2), key=f"FederatedJob/t/o{i}") for i in range(0, 300, 7)]
    assert h.step(T0 + S, events) is None and h.step(T0 + S, events) is None
    ms = ctx.monitor_reconcile_timing() + ctx.monitor_report_timing()
    assert len(ms) == 6 and all(np.isfinite(m) and m >= 0 for m in ms)
    a = M.MonitorBatch.pack(h.table, events[:2], T0).arrays()
    with pytest.raises(runtime.KadError):  # NEW on a live slot
        ctx.monitor_reconcile(**dict(a, obj_flags=a["obj_flags"] | M.NEW))
    with pytest.raises(runtime.KadError):  # a slot twice
        ctx.monitor_reconcile(**dict(a, slot=a["slot"][[0, 0]]))
    assert h.state_diff() is None
    ctx.monitor_clear()
    info = ctx.monitor_info()
    assert info["n_slots"] == 0 and info["n_live"] == 0 and info["capacity"] >= cap + 5000
    assert ctx.monitor_read(slots)["flags"].sum() == 0
    r = ctx.monitor_report(T0, 1)
    assert r["counters"].sum() == 0 and r["n_timers"].tolist() == [0, 0]


def test_schedule_results_are_left_alone(ctx):
    import follower_cases as FC
    snap, fwk, batch, *_ = FC.resident_case()
    ctx.upload_snapshot(snap)
    ctx.upload_batch(batch)
    ctx.schedule(fwk)
    ctx.sync()
    before = ctx.download()
    assert MC.run_seeded(2, device(ctx)) is None
    after = ctx.download()
    ctx.schedule(fwk)
    ctx.sync()
    later = ctx.download()
    for k in ("status", "count", "flags", "cluster", "replicas"):
        assert getattr(before, k).tobytes() == getattr(after, k).tobytes() == getattr(later, k).tobytes(), k


def test_group_member(ctx):
    from kubeadmiral_amd import runtime
    g = runtime.GroupContext([0, 0])
    try:
        assert MC.run_seeded(3, device(g.member(1))) is None
    finally:
        g.close()


def test_end_to_end_through_the_reconciler(ctx):
    """reconcile_monitor over seeded rounds, then monitor_report: the outcomes, the annotated objects and the metrics
    against the checker."""
    from kubeadmiral_amd import objects as O
    from kubeadmiral_amd import synth
    from kubeadmiral_amd.controller import BatchReconciler
    ctx.monitor_clear()
    rec = BatchReconciler(O.FederatedTypeConfig(kind="Deployment"), ctx=ctx)
    ref = R.Monitor()
    for now, events in synth.gen_monitor_events(7, kinds=("FederatedDeployment",), rounds=3):
        name = lambda e: e["key"].split("/", 1)[1]  # noqa: E731
        # what each event saw, aligned with the events: a key's events within the batch differ
        outcomes, updates = rec.reconcile_monitor([(name(e), e["obj"]) for e in events], [e["status"] for e in events],
                                                  [e["members"] for e in events], now)
        want_updates = []
        for e, o in zip(events, outcomes):
            w = ref.reconcile(dict(e, status_enabled=True), R.unix(now))
            assert (o.result, o.update_annotation, o.last_generation, o.meter_deleted) == \
                (w["result"], w["update"], w["last_generation"], w["deleted"])
            if w["update"]:
                want_updates.append((e["obj"]["metadata"]["generation"], w["last_generation"]))
        assert [(u["metadata"]["generation"], u["metadata"]["annotations"]["lastGeneration"]) for u in updates] == want_updates
        assert sorted(rec.monitor_report(now + 6 * MIN)) == ref.metrics(R.unix(now + 6 * MIN))
    # the stores' current objects by name serve as well
    now += MIN
    last = {name(e): e for e in events if e["obj"] is not None}
    outcomes, _ = rec.reconcile_monitor([(n, e["obj"]) for n, e in last.items()], {n: e["status"] for n, e in last.items()},
                                        {n: e["members"] for n, e in last.items()}, now)
    for e, o in zip(last.values(), outcomes):
        assert o.result == ref.reconcile(dict(e, status_enabled=True), R.unix(now))["result"]
    assert sorted(rec.monitor_report(now)) == ref.metrics(R.unix(now))
