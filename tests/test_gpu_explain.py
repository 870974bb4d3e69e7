"""kad_explain (filter_explain_kernel on an MI355X) == the Python oracle's filters applied one plugin at a time.

Expected values: ``oracle.kad_oracle.FILTERS[name](su, cluster)`` in the framework's filter order, the first
plugin that does not succeed takes the cluster (RunFilterPlugins, framework/runtime/framework.go:114-126);
ClusterResourcesFit's short resources come from that result's reasons (fit.go:73-134). Everything is an
integer count or a plugin id, so the comparison is exact.
"""

import functools

import numpy as np
import pytest

from golden_util import case_id, load
from kubeadmiral_amd import framework as F
from kubeadmiral_amd import pack, synth
from kubeadmiral_amd import types as T
from kubeadmiral_amd.results import NOT_REJECTED, PL_FIT
from oracle import kad_oracle as KO

pytestmark = pytest.mark.gpu

DEFAULT = [F.APIResources, F.TaintToleration, F.ClusterResourcesFit, F.PlacementFilter, F.ClusterAffinity]
REVERSED = DEFAULT[::-1]
# (seed, C, n_taints): a single cluster, one short of a chunk, a chunk tail, TW > 1, a partial chunk
CASES = [(1, 1, 9), (2, 63, 9), (3, 65, 9), (4, 130, 130), (5, 40, 9)]
RUNS = [(c, "default") for c in CASES] + [(c, "reversed") for c in CASES if c[0] % 2]


def framework(filters):
    d = F.default_enabled_plugins()
    return F.Framework(F.EnabledPlugins(list(filters), d.score_plugins, d.select_plugins, d.replicas_plugins))


@functools.lru_cache(maxsize=None)
def inputs(seed, C, nt, W=60):
    clusters, units = synth.gen_fuzz(seed, W=W, C=C, n_taints=nt)
    return clusters, units, pack.Snapshot(clusters)


def oracle_explain(clusters, units, filters):
    """(rejected[W][5], feasible[W], fit_detail[W][3], first_fail[W][C]) from the oracle's per-plugin filters."""
    W, C = len(units), len(clusters)
    rej, feas = np.zeros((W, 5), np.int32), np.zeros(W, np.int32)
    fit, ff = np.zeros((W, 3), np.int32), np.full((W, C), NOT_REJECTED, np.uint8)
    for w, su in enumerate(units):
        if su.sticky_cluster and len(su.current_clusters or {}) > 0:  # generic_scheduler.go:101-104
            feas[w] = -1
            continue
        for ci, c in enumerate(clusters):
            for name in filters:
                r = KO.FILTERS[name](su, c)
                if r is None or r.code == KO.SUCCESS:
                    continue
                pl = F.PLUGIN_ID[name]
                rej[w, pl] += 1
                ff[w, ci] = pl
                if pl == PL_FIT:
                    fit[w, 0] += "Insufficient cpu" in r.reasons
                    fit[w, 1] += "Insufficient memory" in r.reasons
                    fit[w, 2] += any(x not in ("Insufficient cpu", "Insufficient memory") for x in r.reasons)
                break
            else:
                feas[w] += 1
    return rej, feas, fit, ff


@functools.lru_cache(maxsize=None)
def expected(case, order):
    clusters, units, _ = inputs(*case)
    return oracle_explain(clusters, units, DEFAULT if order == "default" else REVERSED)


@pytest.fixture(scope="module")
def ctx():
    from kubeadmiral_amd import build, runtime
    build.build()
    c = runtime.Context(0)
    yield c
    c.close()


def upload(ctx, case, fwk):
    clusters, units, snap = inputs(*case)
    batch = pack.Batch(snap, fwk, units)
    ctx.upload_snapshot(snap)
    ctx.upload_batch(batch)
    return clusters, units, snap, batch


def assert_diag(d, want, rows=None):
    rej, feas, fit, ff = want if rows is None else tuple(a[rows] for a in want)
    assert (d.rejected == rej).all(), np.nonzero((d.rejected != rej).any(1))[0][:5]
    assert (d.feasible == feas).all()
    assert (d.fit_detail == fit).all(), np.nonzero((d.fit_detail != fit).any(1))[0][:5]
    if d.first_fail is not None:
        assert (d.first_fail == ff).all(), np.argwhere(d.first_fail != ff)[:5]


@pytest.mark.parametrize("case,order", RUNS, ids=[f"seed{c[0]}-C{c[1]}-{o}" for c, o in RUNS])
def test_explain_matches_oracle(ctx, case, order):
    fwk = framework(DEFAULT if order == "default" else REVERSED)
    clusters, units, snap, batch = upload(ctx, case, fwk)
    # no Resource.sub error in these inputs (their used amounts are map-order dependent in the reference)
    assert not snap.arrays[pack.S_CFLAGS].any()
    C = len(clusters)
    d = ctx.explain(fwk, per_cluster=True)
    assert d.units.tolist() == list(range(len(units))) and d.order == fwk.filter_order()
    assert_diag(d, expected(case, order))
    sticky = np.array([bool(su.sticky_cluster and su.current_clusters) for su in units])
    assert (d.rejected.sum(1) + d.feasible == C)[~sticky].all()
    assert (d.feasible[sticky] == -1).all() and not d.rejected[sticky].any() and not d.fit_detail[sticky].any()
    assert (d.first_fail[sticky] == NOT_REJECTED).all()
    feas_dbg, _ = ctx.debug_scores(fwk)  # the schedule kernel's own AND-ed filter (sticky rows stay zero)
    assert (d.feasible[~sticky] == feas_dbg.sum(1)[~sticky]).all()
    assert ((d.first_fail == NOT_REJECTED)[~sticky] == feas_dbg[~sticky].astype(bool)).all()


def test_staging_buffer_grows_is_reused_and_shrinks():
    """One context: 4 units on C = 3 (with both optional outputs, and with neither: two absent parts), the
    C = 130 case per cluster (about 100x larger), the tiny ones again. Each step equals the oracle, the repeats
    equal the first runs bit for bit; the timer reports KAD_ESTATE before the first call."""
    from kubeadmiral_amd import runtime
    c = runtime.Context(0)

    def timing_ok():
        ms = c.explain_timing()
        assert len(ms) == 2 and all(np.isfinite(t) and t >= 0 for t in ms), ms
    try:
        fwk = framework(DEFAULT)
        tiny, big = (6, 3, 9, 4), CASES[3]
        clusters, units, _, _ = upload(c, tiny, fwk)
        with pytest.raises(runtime.KadError) as e:
            c.explain_timing()
        assert e.value.code == runtime.KAD_ESTATE
        want = oracle_explain(clusters, units, DEFAULT)
        first = c.explain(fwk, per_cluster=True)
        assert_diag(first, want)
        timing_ok()
        bare = c.explain(fwk, units=[2, 0], per_cluster=False, fit_detail=False)
        assert bare.fit_detail is None and bare.first_fail is None
        assert (bare.rejected == want[0][[2, 0]]).all() and (bare.feasible == want[1][[2, 0]]).all()
        timing_ok()
        upload(c, big, fwk)
        assert_diag(c.explain(fwk, per_cluster=True), expected(big, "default"))
        timing_ok()
        upload(c, tiny, fwk)
        again = c.explain(fwk, per_cluster=True)
        for k in ("rejected", "feasible", "fit_detail", "first_fail"):
            assert getattr(again, k).tobytes() == getattr(first, k).tobytes(), k
        bare2 = c.explain(fwk, units=[2, 0], per_cluster=False, fit_detail=False)
        assert bare2.rejected.tobytes() == bare.rejected.tobytes() and bare2.feasible.tobytes() == bare.feasible.tobytes()
        timing_ok()
    finally:
        c.close()


def test_inputs_cover_every_plugin_and_fit_reason():
    """The fuzz inputs exercise what the kernel distinguishes: every plugin is a first failure, every Fit
    resource is short somewhere, and many units have no feasible cluster."""
    rej = sum(expected(c, "default")[0].sum(0) for c in CASES[1:])
    fit = sum(expected(c, "default")[2].sum(0) for c in CASES[1:])
    assert (rej > 0).all() and (fit > 0).all()
    for c in CASES:
        assert int((expected(c, "default")[1] == 0).sum()) >= 30  # of 60 units


def test_window_past_4096_clusters(ctx):
    """C = 4100: 65 chunks, so ClusterAffinity's 64-chunk window is evaluated twice."""
    case = (6, 4100, 9, 8)
    fwk = framework(DEFAULT)
    clusters, units, _, _ = upload(ctx, case, fwk)
    d = ctx.explain(fwk, per_cluster=True)
    want = oracle_explain(clusters, units, DEFAULT)
    assert_diag(d, want)
    assert (want[3][:, 4096:] == F.PLUGIN_ID[F.ClusterAffinity]).any()  # the second window decides something


def test_order_changes_attribution_not_feasibility(ctx):
    case = CASES[2]
    a_fwk, b_fwk = framework(DEFAULT), framework(REVERSED)
    upload(ctx, case, a_fwk)
    a, b = ctx.explain(a_fwk), ctx.explain(b_fwk)
    assert (a.feasible == b.feasible).all()
    assert (a.rejected != b.rejected).any()
    assert (a.rejected.sum(1) == b.rejected.sum(1)).all()


def test_unit_subsets(ctx):
    case = CASES[1]
    fwk = framework(DEFAULT)
    upload(ctx, case, fwk)
    want = expected(case, "default")
    for rows in ([59, 0, 17, 17, 3], [5], list(range(59, -1, -1)), np.arange(0, 60, 7)):
        d = ctx.explain(fwk, rows, per_cluster=True)
        assert d.units.tolist() == list(rows)
        assert_diag(d, want, list(rows))
    d = ctx.explain(fwk, [])
    assert d.rejected.shape == (0, 5) and d.feasible.shape == (0,)
    d = ctx.explain(fwk, [4, 2], fit_detail=False)
    assert d.fit_detail is None and (d.rejected == want[0][[4, 2]]).all()


def test_explain_leaves_schedule_alone(request):
    """explain() before any schedule() equals explain() after one, and the results of a schedule downloaded
    before and after an explain() are the same bytes, as are those of a schedule that follows it."""
    from kubeadmiral_amd import runtime
    case = CASES[3]
    fwk = framework(DEFAULT)
    ctx = runtime.Context(0)  # a context that has never scheduled anything
    request.addfinalizer(ctx.close)
    _, _, _, batch = upload(ctx, case, fwk)
    before = ctx.explain(fwk, per_cluster=True)
    assert_diag(before, expected(case, "default"))
    ctx.schedule(fwk)
    r0 = ctx.download()
    after = ctx.explain(fwk, per_cluster=True)
    for x, y in ((before.rejected, after.rejected), (before.feasible, after.feasible),
                 (before.fit_detail, after.fit_detail), (before.first_fail, after.first_fail)):
        assert x.tobytes() == y.tobytes()
    r1 = ctx.download()
    r2 = ctx.run(fwk, batch)
    for a in ("status", "count", "flags", "cluster", "replicas"):
        assert getattr(r0, a).tobytes() == getattr(r1, a).tobytes() == getattr(r2, a).tobytes(), a


@pytest.mark.parametrize("prof", [2, 3, 0])
def test_filter_subsets(ctx, prof):
    """Profiles that enable some of the filters (in their own order), and none: a plugin that is not enabled
    rejects nothing."""
    case = CASES[4]
    fwk = synth.fuzz_framework(prof)
    clusters, units, _, _ = upload(ctx, case, fwk)
    filters = fwk.enabled.filter_plugins
    d = ctx.explain(fwk, per_cluster=True)
    assert_diag(d, oracle_explain(clusters, units, filters))
    off = [p for n, p in F.PLUGIN_ID.items() if p < 5 and n not in filters]
    assert not d.rejected[:, off].any()
    if not filters:
        sticky = np.array([bool(su.sticky_cluster and su.current_clusters) for su in units])
        assert (d.feasible[~sticky] == len(clusters)).all()


def test_errors(ctx):
    import ctypes

    from kubeadmiral_amd import runtime
    from kubeadmiral_amd.runtime import KadError
    fwk = framework(DEFAULT)
    _, units, _, _ = upload(ctx, CASES[4], fwk)
    W = len(units)
    rej, feas = np.zeros((1, 5), np.int32), np.zeros(1, np.int32)
    view = runtime.ExplainView(rej.ctypes.data, feas.ctypes.data, None, None)
    prof = fwk.to_c()

    def call(order, unit):
        o, u = np.array(order, np.int32), np.array([unit], np.int32)
        return ctx.L.kad_explain(ctx.h, ctypes.byref(prof), o.ctypes.data_as(ctypes.c_void_p), len(order),
                                 u.ctypes.data_as(ctypes.c_void_p), 1, ctypes.byref(view))

    assert call([0, 1, 2, 3, 4], 0) == 0
    for bad in ([0, 1, 2, 3], [0, 1, 2, 3, 3], [0, 1, 2, 3, 5], [0, 1, 2, 3, 4, 4]):  # not a permutation of the mask
        assert call(bad, 0) == -1, bad
    assert call([0, 1, 2, 3, 4], W) == -1 and call([0, 1, 2, 3, 4], -1) == -1
    with pytest.raises(KadError, match="KAD_EINVAL"):
        ctx.explain(fwk, [W])
    with pytest.raises(KadError, match="KAD_EINVAL"):  # a profile the batch was not packed for
        ctx.explain(synth.fuzz_framework(2))
    fresh = runtime.Context(0)
    try:
        fresh.snap, fresh.batch = ctx.snap, ctx.batch  # (sizes for the Python side only: nothing is resident)
        with pytest.raises(KadError, match="KAD_ESTATE"):
            fresh.explain(fwk, [0])
        with pytest.raises(KadError, match="KAD_ESTATE"):
            fresh.explain_timing()
    finally:
        fresh.close()
    assert all(t >= 0 for t in ctx.explain_timing())


FILTERS = load("filters.json")


@pytest.mark.parametrize("c", FILTERS, ids=[case_id(c) for c in FILTERS])
def test_golden_filter_attribution(ctx, c):
    """The reference's own filter test cases, the single plugin enabled: a rejection is that plugin's."""
    su = T.SchedulingUnit.from_json(c["su"])
    su.scheduling_mode = T.SCHEDULING_MODE_DUPLICATE
    su.sticky_cluster = False
    su.max_clusters = None
    cl = T.FederatedCluster.from_json(c["cluster"])
    fwk = F.Framework(F.EnabledPlugins([c["plugin"]], [], [], []))
    snap = pack.Snapshot([cl])
    ctx.upload_snapshot(snap)
    ctx.upload_batch(pack.Batch(snap, fwk, [su]))
    d = ctx.explain(fwk, per_cluster=True)
    pl = F.PLUGIN_ID[c["plugin"]]
    if c["want"] != "Success":
        assert d.rejected[0].tolist() == [int(p == pl) for p in range(5)] and d.feasible[0] == 0
        assert d.first_fail[0, 0] == pl
    else:
        assert d.feasible[0] == 1 and not d.rejected[0].any() and d.first_fail[0, 0] == NOT_REJECTED


@pytest.mark.parametrize("native", [True, False], ids=["native-objects", "python-objects"])
def test_reconcile_diagnosis(native):
    """reconcile(explain=True): an object whose policy matches no cluster gets the rejection counts; without
    explain (the default) every diagnosis stays empty and nothing else differs."""
    import copy
    import re

    from kubeadmiral_amd import objects as O
    from kubeadmiral_amd.controller import BatchReconciler

    ftc, clusters, objs, pols = synth.gen_trigger_workload(np.random.default_rng(5), 40, 16, n_policies=4)
    by_key = {}
    for p in pols:
        if p.spec.auto_migration is not None:
            p.spec.auto_migration.when.pod_unschedulable_for = "2m"
        by_key[(p.namespace, p.name)] = p
    key = O.matched_policy_key(objs[0], True)
    by_key[key].spec.cluster_selector = {"no-such-label": "anywhere"}
    hit = [i for i, o in enumerate(objs) if O.matched_policy_key(o, True) == key]
    plain_objs = copy.deepcopy(objs)
    plain = BatchReconciler(ftc, native_objects=native).reconcile(plain_objs, by_key, clusters)
    got = BatchReconciler(ftc, native_objects=native).reconcile(objs, by_key, clusters, explain=True)
    assert all(g.diagnosis == "" for g in plain)
    assert [(g.stage, g.status, g.result) for g in got] == [(g.stage, g.status, g.result) for g in plain]
    assert objs == plain_objs
    for i, g in enumerate(got):
        no_feasible = g.stage == "scheduled" and g.result.suggested_clusters is None
        assert (g.diagnosis != "") == no_feasible, i
    assert hit
    for i in hit:  # every cluster is some plugin's: "0/16 clusters are available: 9 TaintToleration, 7 ..."
        head, parts = got[i].diagnosis.split(": ", 1)
        assert head == f"0/{len(clusters)} clusters are available", got[i].diagnosis
        counts = [int(x.split()[0]) for x in re.sub(r" \([^)]*\)", "", parts).split(", ")]
        assert sum(counts) == len(clusters), got[i].diagnosis
