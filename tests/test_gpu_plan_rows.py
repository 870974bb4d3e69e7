"""kad_plan_rows and the schedule path's planner kernels against independent references, at the bounds of
kad_plan.h's width switches (int32 / int64 getDesiredPlan and scans, packed / compared sort keys, f64 / go_div
quotient), the lane shapes of the DPP scans, long rows (LDS workspace as routed, global slab), the pair
planner's pairings and the avoid-disruption branches.

The rows are plan_cases.py's; tests/test_plan_ref_host.py shows on the CPU that they are admissible (non-negative,
no wrap, within the reference's round guard — nothing else is sent to a GPU) and that they reach both sides of
every switch. The references are plan_ref.plan_row (the Python oracle's getDesiredPlan) for kad_plan_rows and the
C oracle for the schedule path. Every comparison is exact equality of integers.
"""
import numpy as np
import pytest

import plan_cases as PC
import plan_ref as PR
from gpu_util import assert_same, c_oracle, default_framework
from kubeadmiral_amd import pack
from kubeadmiral_amd import types as T

pytestmark = pytest.mark.gpu

MODES = {"routed": 0, "workspace": 1, "pairs": 2}


@pytest.fixture(scope="module")
def ctx():
    from kubeadmiral_amd import build, runtime
    build.build()
    c = runtime.Context(0)
    yield c
    c.close()


def assert_rows(got, rows, want, what):
    assert len(got) == len(want)
    for i, (g, w, r) in enumerate(zip(got, want, rows)):
        if g == w:
            continue
        for which, a, b in (("plan", g[0], w[0]), ("overflow", g[1], w[1])):
            for j, (x, y) in enumerate(zip(a, b)):
                if x != y:
                    raise AssertionError(
                        f"{what}: row {i} (K={len(r['elems'])} total={r['total']} avoid={r['avoid']} keep={r['keep']}) "
                        f"{which}[{j}]: gpu={x} reference={y}; element {r['elems'][j]}; classify={sorted(PR.classify(r))}")
        raise AssertionError(f"{what}: row {i}: lengths differ")


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("name", [n for n in PC.FAMILIES if n not in PC.DEFAULT_ROUTING_ONLY])
def test_plan_rows_equal_reference(ctx, name, mode):
    """Each family through the routed planners (registers for K <= 64, LDS workspace past it), with every row
    forced through the workspace planner, and with neighbouring rows of K <= 32 through the half-wave pair
    planner: plan and overflow equal plan_ref's."""
    rows, want = PC.family(name)
    ctx.plan_force_workspace(MODES[mode])
    try:
        got = ctx.plan_rows(rows)
    finally:
        ctx.plan_force_workspace(0)
    assert_rows(got, rows, want, f"{name}/{mode}")


@pytest.mark.parametrize("name", PC.DEFAULT_ROUTING_ONLY)
def test_plan_rows_long_rows_equal_reference(ctx, name):
    """K = 257 in the LDS workspace and K = SLAB_K on the global slab (plan_rows_kernel<true>), beside shorter
    rows of the same launch."""
    rows, want = PC.family(name)
    assert_rows(ctx.plan_rows(rows), rows, want, name)


def wide_unit(names):
    """A Divide unit with one weight of 2^31: the batch keeps its i64 preference columns."""
    return T.SchedulingUnit(group="apps", version="v1", kind="Deployment", resource="deployments", namespace="default",
                            name="plan-wide", desired_replicas=1000, scheduling_mode=T.SCHEDULING_MODE_DIVIDE,
                            cluster_names=set(names[:3]), tolerations=[T.Toleration(operator=T.TOLERATION_OP_EXISTS)],
                            weights={names[0]: 1 << 31, names[1]: 5, names[2]: 7})


def test_schedule_path_planner_equals_c_oracle(ctx):
    """plan_pair_kernel, plan_kernel and the workspace planner on Divide units at the planner's bounds, placed
    on 1, 32, 33, 64, 65 and 100 of 100 clusters, desired replicas around 2^24 and up to INT64_MAX: once with the
    i32 preference columns (KAD_BATCH_NARROW_PREFS) and once, beside a unit with a weight of 2^31, with the i64
    columns. Both runs equal the C oracle, and the shared units give the same rows in both."""
    clusters, units, named = PC.schedule_case()
    snap = pack.Snapshot(clusters)
    fwk = default_framework()
    ctx.upload_snapshot(snap)
    results = []
    for extra, flags in (([], pack.BATCH_NARROW_PREFS), ([wide_unit(sorted(c.name for c in clusters))], 0)):
        batch = pack.Batch(snap, fwk, units + extra)
        assert pack.header_of(batch.blob, pack.BatchHeader).flags == flags
        got = ctx.run(fwk, batch)
        counts = ctx.path_counts()
        assert counts["units"] == batch.W and counts["planner_rows"] == batch.W, counts  # every unit is planned
        assert_same(got, c_oracle(snap, batch, fwk), f"planner bounds, batch flags {flags}")
        assert (got.status == pack.ST_OK).all()
        results.append(got)
    narrow, wide = results
    for w in range(len(units)):
        assert narrow.row(w) == wide.row(w) and narrow.flags[w] == wide.flags[w], (w, narrow.row(w), wide.row(w))
    ks = np.array([len(r["elems"]) for r in named])
    assert {int(k) for k in ks} == set(PC.SCHEDULE_KS)  # pair planner, 64-lane planner and workspace planner rows
