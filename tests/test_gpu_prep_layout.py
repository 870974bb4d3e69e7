"""prep_kernel's record store, prologue order and the snapshot's fit fence table == the C oracle, unit by unit.

prep_kernel gives a unit ceil(nch / 4) lanes (nch = ceil(C / 64)); the unit's first lanes store its 64-B
UnitRec in 16-B pieces (4 or more lanes: one piece each, 3 lanes: the third stores two, 2 lanes: two each,
1 lane: all four), every lane loads the unit's batch columns before the block's barrier, and the first
levels of the fit-rank search read a fence table built with the fit values at snapshot upload and update
(prep_wave_kernel, C = 4160, reads the same table). A wrong piece, a lane that stores for its neighbour or a
stale fence changes what the schedule kernels read from the record or the static words, so every case is
compared with the oracle on every unit:

  C     200  lanes per unit 1 (lean route)        448  7 chunks, 2 lanes, the second holds 3
        257  5 chunks, 2 lanes, the second holds 1 512  2 full lanes
        577  10 chunks, 3 lanes                    1000 4 lanes, partial last word (C3's shape)
        4160 prep_wave_kernel<2>
  W     1, 15, 17, 63, 65, 300: a unit's lanes straddle a wave (per = 3) and a block boundary, the last block
        is mostly dead lanes, more than one block

The first units of every batch are one of each kind the record has to carry (KINDS); the fuzz units behind
them mix the same features at random. The inputs are built once per C and the batches are prefixes of one
unit list.
"""

import functools

import numpy as np
import pytest

import gpu_util as G
from gpu_util import assert_same, c_oracle, nch_of
from kubeadmiral_amd import pack, synth
from kubeadmiral_amd import types as T

pytestmark = pytest.mark.gpu

CS = (200, 257, 448, 512, 577, 1000, 4160)
WS = (1, 15, 17, 63, 65, 300)
WIDE_P = 512  # kad_layout.h
KINDS = ("over-request", "row-routed", "sticky", "current", "placement", "scalar", "zero-request", "tiny-request")


def lanes_per_unit(C):
    return (nch_of(C) + 3) // 4


@pytest.fixture(scope="module")
def ctx():
    from kubeadmiral_amd import build, runtime
    build.build()
    c = runtime.Context(0)
    yield c
    c.close()


@functools.lru_cache(maxsize=None)
def inputs(C):
    """(clusters, units, snapshot): one unit of each of KINDS, then gen_fuzz's units."""
    clusters, fuzz = synth.gen_fuzz(8400 + C, W=max(WS), C=C)
    G.serve_deployments(clusters)
    names = [c.name for c in clusters]
    over = G.plain_unit("over-request")  # above every cluster's available amount: the last fit row, nothing feasible
    over.resource_request = T.Resource(1 << 44, 1 << 45)
    routed = G.plain_unit("row-routed")  # every cluster feasible: more than WIDE_P of them at C = 1000
    sticky = G.plain_unit("sticky")
    sticky.sticky_cluster, sticky.current_clusters = True, {names[C // 2]: 2}
    current = G.plain_unit("current")
    current.tolerations = None  # NoExecute taints count on its current clusters only
    current.current_clusters = {names[0]: 1, names[C - 1]: None, names[C // 3]: 4}
    place = G.plain_unit("placement", [names[0], names[63 % C], names[64 % C], names[C - 1]])
    scalar = G.plain_unit("scalar")  # a scalar request: REC_FULL, the full kernel
    scalar.resource_request = T.Resource(100, 1 << 20, 0, {"example.com/gpu": 1})
    zero = G.plain_unit("zero-request")
    zero.resource_request = T.Resource()
    tiny = G.plain_unit("tiny-request")  # below every positive amount: the first fit rows
    tiny.resource_request = T.Resource(1, 1)
    units = [over, routed, sticky, current, place, scalar, zero, tiny]
    assert [u.name for u in units] == list(KINDS)
    return clusters, units + fuzz[:max(WS) - len(units)], pack.Snapshot(clusters)


@functools.lru_cache(maxsize=None)
def layout_case(C, W):
    _, units, snap = inputs(C)
    fwk = G.default_framework()
    batch = pack.Batch(snap, fwk, units[:W])
    return snap, batch, fwk, c_oracle(snap, batch, fwk)


@pytest.fixture
def case(request):
    fn, *args = request.param
    return fn(*args)


def route_id(C):
    nch = nch_of(C)
    return f"C{C}-nch{nch}-" + (f"prepwave{(nch + 63) // 64}" if nch > 64 else f"per{lanes_per_unit(C)}")


@pytest.mark.parametrize("case,C,W", [((layout_case, C, W), C, W) for C in CS for W in WS], indirect=["case"],
                         ids=[f"{route_id(C)}-W{W}" for C in CS for W in WS])
def test_prep_layout_equals_oracle(ctx, case, C, W):
    snap, batch, fwk, want = case
    assert batch.W == W
    ctx.upload_snapshot(snap)
    got = ctx.run(fwk, batch)
    paths, counts, route = ctx.snapshot_paths(), ctx.path_counts(), ctx.last_route()
    assert paths["fold"] and paths["fitfold"], paths  # the fence table is in use
    assert route["prep_lanes"] == lanes_per_unit(C), route
    assert counts["units"] == W, counts
    assert_same(got, want, f"{route_id(C)} W={W}")
    if W >= len(KINDS):
        k = {n: i for i, n in enumerate(KINDS)}
        assert want.count[k["over-request"]] == 0, want.row(k["over-request"])
        assert want.count[k["row-routed"]] == C, want.row(k["row-routed"])
        assert counts["full_kernel"] >= 1, counts  # the scalar request
        if 5 <= nch_of(C) <= 16:  # the wide kernel: lists past its registers are routed to rows by prep
            assert (counts["row_kernel"] >= 1) == (C > WIDE_P), counts


UPDATE_CS = (200, 1000, 4160)


@functools.lru_cache(maxsize=None)
def update_case(C):
    """The C case's snapshot with a third of the clusters' available amounts changed (the informer's status
    update, through the delta), and the oracle on the updated snapshot."""
    clusters, units, _ = inputs(C)
    snap = pack.Snapshot(clusters)  # (its own: update() moves it on)
    fwk = G.default_framework()
    batch = pack.Batch(snap, fwk, units)
    before = c_oracle(snap, batch, fwk)
    new, changed = synth.mutate_clusters(np.random.default_rng(8500 + C), snap.clusters, C // 3, structural=False)
    first = pack.Snapshot(clusters)
    delta = snap.update(new)
    assert delta is not None and len(changed) == C // 3
    return first, delta, snap, batch, fwk, before, c_oracle(snap, batch, fwk)


@pytest.mark.parametrize("case,C", [((update_case, C), C) for C in UPDATE_CS], indirect=["case"],
                         ids=[route_id(C) for C in UPDATE_CS])
def test_fence_table_follows_snapshot_update(ctx, case, C):
    """A snapshot update rebuilds the fit values, so the fences must be rebuilt with them: the resident batch
    scheduled after the update equals the oracle on the updated snapshot."""
    first, delta, snap, batch, fwk, before, after = case
    assert not (before.equal_rows(after) & (before.flags == after.flags)).all()  # the update changes results
    ctx.upload_snapshot(first)
    assert_same(ctx.run(fwk, batch), before, f"{route_id(C)} before the update")
    ctx.update_snapshot(delta)
    assert ctx.snapshot_paths()["fitfold"]
    ctx.schedule(fwk)  # resident batch, no re-upload
    assert_same(ctx.download(), after, f"{route_id(C)} after the update")
