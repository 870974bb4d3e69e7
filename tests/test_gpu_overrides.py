"""kad_override_match on an MI355X == the object-by-object checker (override_ref.py), exactly: every status and
every word of every matched row are integers.

Shapes: C in {1, 63, 65, 130, 4100} — a single cluster, one short of a chunk, a chunk tail, three chunks, and more
than 64 chunks; ~200 objects over ~40 fuzz policies of 0-6 rules plus one rule of each kind
(override_ref.special_policies) and one object whose two policies hold more than 32 rules (RW = 2); placed
lists of 0..min(C, 12) clusters including the unknown id -1."""

import copy
import functools
import json
import os

import numpy as np
import pytest

import override_ref as R
from kubeadmiral_amd import framework as F
from kubeadmiral_amd import overrides as OV
from kubeadmiral_amd import pack, synth
from kubeadmiral_amd import types as T

pytestmark = pytest.mark.gpu

CASES = [(1, 1), (2, 63), (3, 65), (4, 130), (5, 4100)]
HERE = os.path.dirname(os.path.abspath(__file__))
with open(os.path.join(HERE, "golden", "override_policy.json")) as _f:
    GOLDEN = json.load(_f)


@pytest.fixture(scope="module")
def ctx():
    from kubeadmiral_amd import build, runtime
    build.build()
    c = runtime.Context(0)
    yield c
    c.close()


@functools.lru_cache(maxsize=None)
def inputs(seed, C, n_obj=200):
    """(clusters, snapshot, policies, obj_policy, place_off, place_cluster, RW, checker status, checker rows)."""
    clusters, _ = synth.gen_fuzz(seed, W=1, C=C)
    pols = synth.gen_override_policies(seed, clusters)
    special, _ = R.special_policies(clusters)
    for p in special[3::2]:  # some of the failing kinds as OverridePolicies: the second policy can fail too
        p.namespace = "ns"
    patch = OV.JsonPatchOverrider("replace", "/spec/big", b"2")
    big = [OV.OverridePolicy(f"big-{k}", ns, [OV.OverrideRule(
        OV.TargetClusters(cluster_selector={f"key{j % 4}": f"val{(j + k) % 3}"}) if j % 3 else None, [patch])
        for j in range(20)]) for k, ns in enumerate((None, "ns"))]
    pols = pols + special + big
    cp = [i for i, p in enumerate(pols[:-2]) if not p.namespace]
    npol = [i for i, p in enumerate(pols[:-2]) if p.namespace]
    rng = np.random.default_rng([seed, 77])
    op = np.full((n_obj, 2), -1, np.int32)
    placed = []
    for i in range(n_obj):
        if rng.random() < 0.75:
            op[i][0] = cp[int(rng.integers(len(cp)))]
        if rng.random() < 0.75:
            op[i][1] = npol[int(rng.integers(len(npol)))]
        k = int(rng.integers(0, min(C, 12) + 1))
        ids = [int(c) for c in rng.choice(C, k, replace=False)]
        if rng.random() < 0.15:
            ids.insert(int(rng.integers(0, len(ids) + 1)), -1)
        placed.append(ids)
    op[0] = (len(pols) - 2, len(pols) - 1)  # 40 rules: RW = 2
    off = np.zeros(n_obj + 1, np.int32)
    off[1:] = np.cumsum([len(p) for p in placed])
    ids = np.array([c for p in placed for c in p], np.int32)
    snap = pack.Snapshot(clusters)
    rw = 2
    status, rows = R.expected_match(pols, op, off, ids, clusters, rw)
    return clusters, snap, pols, op, off, ids, rw, status, rows


@functools.lru_cache(maxsize=None)
def checker_conditions():
    """Across the cases, on the checker's output alone: objects with status 0, 1 and 2; at least a tenth of the
    OK objects have a slot with no matched rule, at least a tenth a slot with two or more."""
    seen, ok, none, two = set(), 0, 0, 0
    for case in CASES:
        _, _, _, op, off, ids, _, status, rows = inputs(*case)
        seen |= set(int(s) for s in status)
        for i in np.nonzero(status == 0)[0]:
            cnt = [sum(bin(int(w)).count("1") for w in rows[s]) for s in range(off[i], off[i + 1]) if ids[s] >= 0]
            ok += 1
            none += any(c == 0 for c in cnt)
            two += any(c >= 2 for c in cnt)
    return seen, ok, none, two


def upload(ctx, snap, pols):
    ctx.upload_snapshot(snap)
    pset = OV.PolicySet(snap, pols)
    ctx.upload_override_policies(pset)
    return pset


def test_checker_conditions():
    seen, ok, none, two = checker_conditions()
    assert seen == {0, 1, 2}
    assert none * 10 >= ok and two * 10 >= ok, (ok, none, two)


@pytest.mark.parametrize("case", CASES, ids=[f"C{c}" for _, c in CASES])
def test_fuzz_parity(ctx, case):
    seen, ok, none, two = checker_conditions()
    assert seen == {0, 1, 2} and none * 10 >= ok and two * 10 >= ok
    clusters, snap, pols, op, off, ids, rw, status, rows = inputs(*case)
    pset = upload(ctx, snap, pols)
    assert pset.rule_words(op) == rw and np.diff(pset.arrays[OV.O_RULE_PROG_OFF]).max() > 64
    got_status, got_rows = ctx.override_match(op, (off, ids), rule_words=rw)
    assert (got_status == status).all(), np.nonzero(got_status != status)[0][:5]
    assert (got_rows == rows).all(), np.nonzero((got_rows != rows).any(1))[0][:5]
    from kubeadmiral_amd.runtime import KadError
    with pytest.raises(KadError):  # object 0 holds 40 rules
        ctx.override_match(op, (off, ids), rule_words=1)
    assert all(t >= 0 for t in ctx.override_timing())


def test_golden_cases_on_device(ctx):
    for case in GOLDEN["TestIsClusterMatched"]:
        cl = R.cluster_from_json(case["cluster"])
        pol = OV.OverridePolicy("p", None, [OV.OverrideRule(R.target_from_json(case["targetClusters"]), [])])
        upload(ctx, pack.Snapshot([cl]), [pol])
        st, rows = ctx.override_match([[0, -1]], ([0, 1], [0]))
        assert st[0] == 0 and bool(rows[0][0] & 1) == case["shouldMatch"], case["name"]
    for case in GOLDEN["TestParseOverrides"]:
        cls = [R.cluster_from_json(c) for c in case["clusters"]]
        snap = pack.Snapshot(cls)
        pset = upload(ctx, snap, [R.policy_from_json(case["policy"])])
        n = len(cls)
        st, rows = ctx.override_match([[-1, 0]], ([0, n], list(range(n))))
        assert (st[0] == 2) == case["isErrorExpected"], case["name"]
        got = OV.assemble(pset, np.array([[-1, 0]]), [0, n], [c.name for c in cls], st, rows)[0]
        if case["isErrorExpected"]:
            assert isinstance(got, OV.OverrideError) and not rows.any()
        else:
            assert got == R.map_from_json(case["expected"]), case["name"]


def test_placed_clusters_from_results(ctx):
    clusters, units = synth.gen_fuzz(11, W=120, C=40)
    fwk = F.Framework(F.default_enabled_plugins())
    snap = pack.Snapshot(clusters)
    batch = pack.Batch(snap, fwk, units)
    pols = synth.gen_override_policies(11, clusters) + R.special_policies(clusters)[0]
    upload(ctx, snap, pols)
    from kubeadmiral_amd.runtime import KadError
    ctx.upload_batch(batch)
    with pytest.raises(KadError) as e:  # nothing scheduled yet
        ctx.override_match(np.full((len(units), 2), -1, np.int32))
    assert e.value.code == -4
    ctx.schedule(fwk)
    before = ctx.download()
    st = before.status
    dup = np.array([u.scheduling_mode == T.SCHEDULING_MODE_DUPLICATE for u in units])
    assert (st == pack.ST_STICKY).any() and (st == pack.ST_NO_FEASIBLE).any()
    assert ((st == pack.ST_OK) & dup & (before.count > 0)).any() and ((st == pack.ST_OK) & ~dup & (before.count > 0)).any()
    W = len(units)
    rng = np.random.default_rng(11)
    op = np.stack([rng.integers(-1, len(pols), W), rng.integers(-1, len(pols), W)], 1).astype(np.int32)
    rw = OV.PolicySet(snap, pols).rule_words(op)
    got_status, got_rows = ctx.override_match(op, None, rule_words=rw)
    # the same placements, explicit: unit i's output slots, or its CurrentClusters entries when sticky
    cur_off, cur_id = batch.arrays[pack.B_CUR_OFF], batch.arrays[pack.B_CUR_ID]
    n_out = batch.n_out_slots
    assert len(got_rows) == n_out + len(cur_id)
    slots = []
    for i in range(W):
        if st[i] == pack.ST_OK:
            slots.append(list(range(int(batch.out_off[i]), int(batch.out_off[i]) + int(before.count[i]))))
        elif st[i] == pack.ST_STICKY:
            slots.append(list(range(n_out + int(cur_off[i]), n_out + int(cur_off[i + 1]))))
        else:
            slots.append([])
    cluster_of = np.concatenate([before.cluster[:n_out], cur_id]) if n_out + len(cur_id) else np.zeros(0, np.int32)
    off = np.zeros(W + 1, np.int32)
    off[1:] = np.cumsum([len(s) for s in slots])
    flat = np.array([s for ss in slots for s in ss], np.int64)
    ids = cluster_of[flat].astype(np.int32)
    assert len(ids) > W // 2
    ex_status, ex_rows = ctx.override_match(op, (off, ids), rule_words=rw)
    want_status, want_rows = R.expected_match(pols, op, off, ids, clusters, rw)
    assert (ex_status == want_status).all() and (ex_rows == want_rows).all()
    assert (got_status == want_status).all()
    assert (got_rows[flat] == want_rows).all()
    rest = np.ones(len(got_rows), bool)
    rest[flat] = False
    assert not got_rows[rest].any()  # slots that hold no placed cluster
    assert (want_status != 0).any() and (want_status == 0).any()
    # the results are untouched, and a later schedule gives them again
    after = ctx.download()
    for a, b in zip((before.status, before.count, before.flags, before.cluster, before.replicas),
                    (after.status, after.count, after.flags, after.cluster, after.replicas)):
        assert a.tobytes() == b.tobytes()
    ctx.schedule(fwk)
    again = ctx.download()
    for a, b in zip((before.status, before.count, before.flags, before.cluster, before.replicas),
                    (again.status, again.count, again.flags, again.cluster, again.replicas)):
        assert a.tobytes() == b.tobytes()


def _timing_ok(ms):
    assert len(ms) == 3 and all(np.isfinite(t) and t >= 0 for t in ms), ms


def test_staging_buffer_explicit_small_large_small():
    """One context, explicit placements: 3 objects on C = 3 with n_slots = 0 and with their own placements, the
    200-object C = 65 case, the tiny ones again. Each step equals the checker, the repeats equal the first runs
    bit for bit; the timer reports KAD_ESTATE before the first call."""
    from kubeadmiral_amd import runtime
    c = runtime.Context(0)
    try:
        clusters, snap, pols, op, off, ids, rw, status, rows = inputs(6, 3, 3)
        upload(c, snap, pols)
        with pytest.raises(runtime.KadError) as e:
            c.override_timing()
        assert e.value.code == runtime.KAD_ESTATE
        off0, ids0 = np.zeros(len(op) + 1, np.int32), np.zeros(0, np.int32)
        status0, rows0 = R.expected_match(pols, op, off0, ids0, clusters, rw)
        first0 = c.override_match(op, (off0, ids0), rule_words=rw)
        assert (first0[0] == status0).all() and len(first0[1]) == 0 == len(rows0)
        _timing_ok(c.override_timing())
        first = c.override_match(op, (off, ids), rule_words=rw)
        assert (first[0] == status).all() and (first[1] == rows).all()
        _, bsnap, bpols, bop, boff, bids, brw, bstatus, brows = inputs(3, 65)
        assert len(bids) >= 30 * max(1, len(ids))
        upload(c, bsnap, bpols)
        big = c.override_match(bop, (boff, bids), rule_words=brw)
        assert (big[0] == bstatus).all() and (big[1] == brows).all()
        _timing_ok(c.override_timing())
        upload(c, snap, pols)
        for want, placed in ((first0, (off0, ids0)), (first, (off, ids))):
            again = c.override_match(op, placed, rule_words=rw)
            assert again[0].tobytes() == want[0].tobytes() and again[1].tobytes() == want[1].tobytes()
            _timing_ok(c.override_timing())
    finally:
        c.close()


def _results_case(W, C):
    clusters, units = synth.gen_fuzz(11, W=W, C=C)
    fwk = F.Framework(F.default_enabled_plugins())
    snap = pack.Snapshot(clusters)
    pols = synth.gen_override_policies(11, clusters) + R.special_policies(clusters)[0]
    rng = np.random.default_rng([11, W])
    op = np.stack([rng.integers(-1, len(pols), W), rng.integers(-1, len(pols), W)], 1).astype(np.int32)
    return clusters, fwk, snap, pack.Batch(snap, fwk, units), pols, op


def _match_results(c, case):
    """kad_override_match on the last schedule's placements, checked against the checker on the same placements
    written out (unit i's output slots, or its CurrentClusters entries when sticky); returns what it gave."""
    clusters, fwk, snap, batch, pols, op = case
    upload(c, snap, pols)
    res = c.run(fwk, batch)
    W, n_out = len(op), batch.n_out_slots
    rw = OV.PolicySet(snap, pols).rule_words(op)
    got_status, got_rows = c.override_match(op, None, rule_words=rw)
    cur_off, cur_id = batch.arrays[pack.B_CUR_OFF], batch.arrays[pack.B_CUR_ID]
    slots = []
    for i in range(W):
        if res.status[i] == pack.ST_OK:
            slots.append(list(range(int(batch.out_off[i]), int(batch.out_off[i]) + int(res.count[i]))))
        elif res.status[i] == pack.ST_STICKY:
            slots.append(list(range(n_out + int(cur_off[i]), n_out + int(cur_off[i + 1]))))
        else:
            slots.append([])
    cluster_of = np.concatenate([res.cluster[:n_out], cur_id]).astype(np.int32)
    off = np.zeros(W + 1, np.int32)
    off[1:] = np.cumsum([len(x) for x in slots])
    flat = np.array([x for ss in slots for x in ss], np.int64)
    want_status, want_rows = R.expected_match(pols, op, off, cluster_of[flat].astype(np.int32), clusters, rw)
    assert (got_status == want_status).all()
    assert (got_rows[flat] == want_rows).all()
    rest = np.ones(len(got_rows), bool)
    rest[flat] = False
    assert not got_rows[rest].any()
    _timing_ok(c.override_timing())
    return got_status, got_rows


def test_staging_buffer_from_results_small_large_small(ctx):
    """One context, the placements of the last schedule: 3 units on C = 3, 300 units on C = 40, the 3 again —
    each equal to the checker, the third equal to the first bit for bit."""
    tiny, big = _results_case(3, 3), _results_case(300, 40)
    first = _match_results(ctx, tiny)
    _match_results(ctx, big)
    again = _match_results(ctx, tiny)
    assert again[0].tobytes() == first[0].tobytes() and again[1].tobytes() == first[1].tobytes()


def test_snapshot_update_moves_a_label(ctx):
    clusters, snap0, pols, op, off, ids, rw, status, rows = inputs(3, 65)
    snap = pack.Snapshot(clusters)  # (the cached one stays as packed)
    upload(ctx, snap, pols)
    new = copy.deepcopy(clusters)
    donors = {}
    moved = 0
    for c in new:  # rotate key0's values among the clusters that have it: known values, new holders
        if c.labels and "key0" in c.labels:
            donors.setdefault(c.labels["key0"], c)
    vals = sorted(donors)
    assert len(vals) >= 2
    for c in new:
        if c.labels and "key0" in c.labels and moved < 20:
            c.labels["key0"] = vals[(vals.index(c.labels["key0"]) + 1) % len(vals)]
            moved += 1
    delta = snap.diff(new)
    assert delta is not None and len(delta.changed) == moved
    ctx.update_snapshot(delta)
    snap.commit(delta)
    got_status, got_rows = ctx.override_match(op, (off, ids), rule_words=rw)
    want_status, want_rows = R.expected_match(pols, op, off, ids, new, rw)
    assert (want_rows != rows).any()  # the move is visible to the checker
    assert (got_status == want_status).all() and (got_rows == want_rows).all()
    upload(ctx, pack.Snapshot(new), pols)  # a fresh upload of the new clusters
    f_status, f_rows = ctx.override_match(op, (off, ids), rule_words=rw)
    assert (f_status == got_status).all() and (f_rows == got_rows).all()


def test_upload_refused_against_another_snapshot(ctx):
    clusters, snap, pols = inputs(2, 63)[:3]
    other = pack.Snapshot(synth.gen_fuzz(9, W=1, C=63)[0])
    ctx.upload_snapshot(other)
    from kubeadmiral_amd.runtime import KadError
    with pytest.raises(KadError) as e:
        ctx.upload_override_policies(OV.PolicySet(snap, pols))
    assert e.value.code == -1


def test_host_assembly(ctx):
    clusters, snap, pols, op, off, ids, rw, status, rows = inputs(4, 130)
    ctx.upload_snapshot(snap)
    m = OV.OverrideMatcher(ctx, snap, pols)
    objs, namespaced, placed, chains = [], [], [], []
    for i in range(len(op)):
        labels = {}
        chain = []
        if op[i][0] >= 0:
            labels[OV.CLUSTER_OVERRIDE_POLICY_NAME_LABEL] = pols[op[i][0]].name
            chain.append(pols[op[i][0]])
        if op[i][1] >= 0:
            labels[OV.OVERRIDE_POLICY_NAME_LABEL] = pols[op[i][1]].name
            chain.append(pols[op[i][1]])
        objs.append({"metadata": {"namespace": "ns", "name": f"o{i}", "labels": labels}, "spec": {}})
        namespaced.append(True)
        placed.append([clusters[c].name if c >= 0 else "ghost-cluster" for c in ids[off[i]:off[i + 1]]])
        chains.append(chain)
    objs[1]["metadata"]["labels"][OV.OVERRIDE_POLICY_NAME_LABEL] = "no-such-policy"
    got = m.match(objs, namespaced, placed)
    assert got[1] == OV.OverrideError(OV.MATCH_FAILED, None, "")
    n_err = n_map = 0
    for i in range(len(op)):
        if i == 1:
            continue
        want, fail_at = R.merged_overrides(chains[i], [clusters[c] for c in ids[off[i]:off[i + 1]] if c >= 0])
        if fail_at >= 0:
            assert got[i] == OV.OverrideError(OV.PARSE_FAILED, chains[i][fail_at].key(), ""), i
            n_err += 1
        else:
            assert got[i] == want, i
            n_map += bool(want)
            assert OV.apply(objs[i], got[i]) == bool(want)
    assert n_err and n_map
