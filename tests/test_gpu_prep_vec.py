"""prep_kernel's 16-byte row accesses (route PREP_VEC) == the C oracle, unit by unit, and the routes beside it.

Where a snapshot has a multiple of four 64-cluster chunks and every row table starts on a 16-byte boundary,
prep_kernel<true> reads a lane's four words of a requirement row, of the two fit rows, of the taint table's
rows (both tables) and of the GVK slice as two 16-byte loads, and stores its static and current-cluster words
as two 16-byte stores. A wrong word order, a lane reading its neighbour's words or a lost tail mask changes
the static words, so every unit's result is compared with the oracle through the public schedule path.

  C   vector route   256  4 chunks, one lane per unit, lean kernel     450  8 chunks, ragged last chunk
                     705  12 chunks, three lanes per unit              1000 16 chunks (C3's shape)
      scalar route   300  5 chunks                                      960  15 chunks
  W   1, 63, 65, 257: the last block has dead lanes, a unit's lanes sit at the start and the end of a block,
      more than one block

The first units of every batch use one vectorised access each (KINDS); gen_fuzz's units behind them (40 taint
ids: five 8-id groups of the taint table) mix the features at random. The route is asserted from
kad_last_route, so a batch that silently took the other form fails.
"""

import functools

import pytest

import gpu_util as G
from gpu_util import assert_same, c_oracle, nch_of
from kubeadmiral_amd import pack, synth
from kubeadmiral_amd import types as T

pytestmark = pytest.mark.gpu

VEC_CS = (256, 450, 705, 1000)
SCALAR_CS = (300, 960)
WS = (1, 63, 65, 257)
KINDS = ("selector-3", "required-3-exprs", "request", "placement", "current-no-tolerations", "tolerates-four-keys",
         "gvk-nowhere", "gvk-everywhere", "gvk-somewhere")


@pytest.fixture(scope="module")
def ctx():
    from kubeadmiral_amd import build, runtime
    build.build()
    c = runtime.Context(0)
    yield c
    c.close()


@functools.lru_cache(maxsize=None)
def inputs(C):
    """(units, snapshot): one unit per entry of KINDS, then gen_fuzz's."""
    clusters, fuzz = synth.gen_fuzz(9100 + C, W=max(WS), C=C, n_taints=40)
    G.serve_deployments(clusters)
    names = [c.name for c in clusters]
    labelled = next(c for c in clusters if c.labels and len(c.labels) >= 3)
    sel = G.plain_unit("selector-3")  # three ClusterSelector entries: three requirement rows ANDed
    sel.cluster_selector = dict(list(labelled.labels.items())[:3])
    req = G.plain_unit("required-3-exprs")  # two terms, the first with three expressions
    keys = list(labelled.labels)[:3]
    req.affinity = T.Affinity(T.ClusterAffinity(T.ClusterSelector([
        T.ClusterSelectorTerm([T.ClusterSelectorRequirement(k, T.OP_EXISTS, None) for k in keys], None),
        T.ClusterSelectorTerm([T.ClusterSelectorRequirement(keys[0], T.OP_NOT_IN, [labelled.labels[keys[0]]]),
                               T.ClusterSelectorRequirement(keys[1], T.OP_EXISTS, None)], None)]), None))
    fit = G.plain_unit("request")  # a non-zero request: the two fit rows
    fit.resource_request = T.Resource(2000, 4 * synth.GI)
    place = G.plain_unit("placement", [names[0], names[63 % C], names[64 % C], names[C // 2], names[C - 1]])
    cur = G.plain_unit("current-no-tolerations")  # every present taint group untolerated, NoExecute table on cw
    cur.tolerations = None
    cur.current_clusters = {names[0]: 1, names[C - 1]: None, names[C // 3]: 4, names[(2 * C) // 3]: 2}
    # 4 of the 13 taint keys tolerated: at least 27 of the 40 ids stay untolerated, which no three 8-id groups hold
    tol = G.plain_unit("tolerates-four-keys")
    tol.tolerations = [T.Toleration(f"taint-{i}", T.TOLERATION_OP_EXISTS, "", "") for i in range(4)]
    tol.current_clusters = {names[1 % C]: 3}
    nowhere = G.plain_unit("gvk-nowhere")
    nowhere.group, nowhere.version, nowhere.kind = synth.GVKS[3]
    everywhere = G.plain_unit("gvk-everywhere")  # (serve_deployments)
    somewhere = G.plain_unit("gvk-somewhere")
    somewhere.group, somewhere.version, somewhere.kind = synth.GVKS[1]
    units = [sel, req, fit, place, cur, tol, nowhere, everywhere, somewhere]
    assert [u.name for u in units] == list(KINDS)
    served = [sum(any((a.group, a.version, a.kind) == g for a in c.api_resource_types or []) for c in clusters)
              for g in (synth.GVKS[3], synth.GVKS[0], synth.GVKS[1])]
    assert served[0] == 0 and served[1] == C and 0 < served[2] < C, served
    return units + fuzz[:max(WS) - len(units)], pack.Snapshot(clusters)


@functools.lru_cache(maxsize=None)
def vec_case(C, W):
    units, snap = inputs(C)
    fwk = G.default_framework()
    batch = pack.Batch(snap, fwk, units[:W])
    return snap, batch, fwk, c_oracle(snap, batch, fwk)


@pytest.fixture
def case(request):
    fn, *args = request.param
    return fn(*args)


def run_and_compare(ctx, case, C, W, prep):
    snap, batch, fwk, want = case
    assert batch.W == W
    ctx.upload_snapshot(snap)
    got = ctx.run(fwk, batch)
    paths, counts, route = ctx.snapshot_paths(), ctx.path_counts(), ctx.last_route()
    assert paths["fold"] and paths["fitfold"], paths  # the taint table, the slices and the fit rows are read
    assert route["prep"] == prep, route
    assert route["prep_lanes"] == (nch_of(C) + 3) // 4, route
    assert route["family"] == ("LEAN" if nch_of(C) <= 4 else "WIDE"), route
    assert counts["units"] == W, counts
    assert_same(got, want, f"C={C} W={W} {prep}")
    if W >= len(KINDS):
        k = {n: i for i, n in enumerate(KINDS)}
        assert want.count[k["gvk-nowhere"]] == 0, want.row(k["gvk-nowhere"])
        assert want.count[k["gvk-everywhere"]] == C, want.row(k["gvk-everywhere"])
        assert 0 < want.count[k["gvk-somewhere"]] < C, want.row(k["gvk-somewhere"])
        assert 0 < want.count[k["placement"]] <= 5, want.row(k["placement"])
        assert want.count[k["current-no-tolerations"]] < C, want.row(k["current-no-tolerations"])


@pytest.mark.parametrize("case,C,W", [((vec_case, C, W), C, W) for C in VEC_CS for W in WS], indirect=["case"],
                         ids=[f"C{C}-nch{nch_of(C)}-W{W}" for C in VEC_CS for W in WS])
def test_vector_route_equals_oracle(ctx, case, C, W):
    assert nch_of(C) % 4 == 0
    run_and_compare(ctx, case, C, W, "PREP_VEC")


@pytest.mark.parametrize("case,C,W", [((vec_case, C, W), C, W) for C in SCALAR_CS for W in WS], indirect=["case"],
                         ids=[f"C{C}-nch{nch_of(C)}-W{W}" for C in SCALAR_CS for W in WS])
def test_scalar_route_beside_it_equals_oracle(ctx, case, C, W):
    assert nch_of(C) % 4 != 0
    run_and_compare(ctx, case, C, W, "PREP")
