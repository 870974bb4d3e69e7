"""kad_follower_union on an MI355X == the object-by-object checker (follower_ref.py), exactly: changed, count,
out_off and out_cluster are integers.

Shapes (follower_cases.py): n_ids in {1, 63, 64, 65, 130, 4100, 8192, 8193, 70000} — one word, a word tail,
the wave path's largest id space, the first of the block path, and ids far past the snapshot's clusters;
0, 1, 2 and 65 leaders per follower; leader lists of 0, 1, 64, 65 and 300 ids with duplicates; an absent
leader, a leader twice, an unchanged placement in another order with duplicates, the two empty-union cases."""
import copy

import numpy as np
import pytest

import follower_cases as FC
import follower_ref as R
from kubeadmiral_amd import follower as FL
from kubeadmiral_amd import objects as O
from kubeadmiral_amd import pack, synth

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from kubeadmiral_amd import build, runtime
    build.build()
    c = runtime.Context(0)
    yield c
    c.close()


def small_snapshot(C):
    clusters, _ = synth.gen_fuzz(11, W=1, C=C)
    return pack.Snapshot(clusters)


def assert_equal(got, want):
    changed, count, off, out = want
    assert (got["changed"] == changed).all(), np.nonzero(got["changed"] != changed)[0][:5]
    assert (got["count"] == count).all(), np.nonzero(got["count"] != count)[0][:5]
    assert (got["out_off"] == off).all(), np.nonzero(got["out_off"] != off)[0][:5]
    assert len(got["out_cluster"]) == len(out) and (got["out_cluster"] == out).all()


@pytest.mark.parametrize("n_ids", FC.N_IDS)
def test_explicit_parity(ctx, n_ids):
    lead, sets, fol, shapes = FC.explicit_case(n_ids)
    ctx.upload_snapshot(small_snapshot(130 if n_ids == 70000 else 1))  # 70000: ids far past the snapshot's C
    got = ctx.follower_union(n_ids, fol, leaders=lead)
    assert_equal(got, R.union_batch(fol, sets))
    route = ctx.follower_last_route()
    assert route["path"] == ("WAVE" if n_ids <= 8192 else "BLOCK") and route["words"] == (n_ids + 31) // 32
    assert got["changed"][shapes["delete"]] == 1 and got["count"][shapes["delete"]] == 0
    assert got["changed"][shapes["nothing"]] == 0 and got["changed"][shapes["same-set-other-order"]] == 0
    # every follower's union, ascending, against the default emit (changed followers only)
    every = ctx.follower_union(n_ids, fol, leaders=lead, emit_all=True)
    assert_equal(every, R.union_batch(fol, sets, emit_all=True))
    assert (every["changed"] == got["changed"]).all() and (np.diff(every["out_off"]) == every["count"]).all()
    for i in np.nonzero(got["changed"])[0]:
        a = got["out_cluster"][got["out_off"][i]:got["out_off"][i + 1]]
        assert (a == every["out_cluster"][every["out_off"][i]:every["out_off"][i + 1]]).all()
        assert (np.diff(a) > 0).all()
    assert all(t >= 0 for t in ctx.follower_timing())


def test_capacity_too_small_then_retry(ctx):
    from kubeadmiral_amd import runtime
    lead, sets, fol, _ = FC.explicit_case(4100)
    want = R.union_batch(fol, sets)
    ctx.upload_snapshot(small_snapshot(1))
    with pytest.raises(runtime.KadError) as e:
        ctx.follower_union(4100, fol, leaders=lead, capacity=int(want[2][-1]) - 1, retry=False)
    assert e.value.code == runtime.KAD_ENOSPC
    for k, w in zip(("changed", "count", "out_off"), want):  # still valid: the caller sizes its retry from them
        assert (e.value.partial[k] == w).all(), k
    got = ctx.follower_union(4100, fol, leaders=lead, capacity=0)
    assert got["calls"] == 2
    assert_equal(got, want)
    assert ctx.follower_union(4100, fol, leaders=lead, capacity=int(want[2][-1]))["calls"] == 1


def test_alternating_large_and_subset_twice(ctx):
    """Consecutive followers of one wave alternate between a large union and a strict subset of it: a word
    left set by the touched-word clear would show as extra ids. Twice on one context: identical output."""
    ctx.upload_snapshot(small_snapshot(1))
    # the stride of a saturated grid on this device: from a batch of followers without leaders
    n = 40000
    z = np.zeros(n + 1, np.int32)
    ctx.follower_union(1000, (z, z[:0], z, z[:0], np.zeros(n, np.uint8)), leaders=FC.csr([[]]))
    stride = ctx.follower_last_route()["stride"]
    assert 0 < stride < n
    lead, sets, fol = FC.alternating_case(stride)
    F = len(fol[4])
    assert F >= 1000 and F >= 3 * stride
    a = ctx.follower_union(1000, fol, leaders=lead)
    route = ctx.follower_last_route()
    assert route["path"] == "WAVE" and route["stride"] == stride  # every wave: large, subset, large
    assert_equal(a, R.union_batch(fol, sets))
    rounds = (np.arange(F) // stride) % 2
    assert a["count"][rounds == 1].max() <= 5 < 40 <= a["count"][rounds == 0].min()
    b = ctx.follower_union(1000, fol, leaders=lead)
    for k in ("changed", "count", "out_off", "out_cluster"):
        assert (a[k] == b[k]).all(), k


def test_resident_mode(ctx):
    snap, fwk, batch, n_ids, L, keep, sched, fol = FC.resident_case()
    ctx.upload_snapshot(snap)
    res = ctx.run(fwk, batch)
    classes = FC.status_classes(res.status)
    assert all(classes.values()), classes
    hdr = pack.header_of(batch.blob, pack.BatchHeader)
    cur_off = pack.array_of(batch.blob, hdr, pack.B_CUR_OFF, np.int32, hdr.n_units + 1)
    cur_id = pack.array_of(batch.blob, hdr, pack.B_CUR_ID, np.int32, int(cur_off[-1]))
    sets = R.resident_leader_sets(res.status, res.count, res.cluster, batch.out_off, cur_off, cur_id, L, sched, keep)
    got = ctx.follower_union(n_ids, fol, keep=keep, sched=sched, n_leaders=L)
    assert_equal(got, R.union_batch(fol, sets))
    # sched_* is read for error-status units only: junk everywhere else changes nothing
    junk_rows = [[int(x) for x in sched[1][sched[0][w]:sched[0][w + 1]]] if res.status[w] >= 3 else [n_ids - 1, 0, n_ids - 2]
                 for w in range(len(res.status))]
    junk = ctx.follower_union(n_ids, fol, keep=keep, sched=FC.csr(junk_rows), n_leaders=L)
    for k in ("changed", "count", "out_off", "out_cluster"):
        assert (junk[k] == got[k]).all(), k
    # and it matters for them: without sched the error units' followers lose those clusters
    none = ctx.follower_union(n_ids, fol, keep=keep, n_leaders=L)
    sets0 = R.resident_leader_sets(res.status, res.count, res.cluster, batch.out_off, cur_off, cur_id, L, None, keep)
    assert_equal(none, R.union_batch(fol, sets0))
    assert (none["count"] != got["count"]).any()
    # the resident results are as they were
    again = ctx.download()
    assert (again.status == res.status).all() and (again.cluster == res.cluster).all()


def _assert_timing(ms):
    assert len(ms) >= 2 and all(np.isfinite(t) and t >= 0 for t in ms), ms


def test_staging_buffer_grows_is_reused_and_shrinks():
    """One context: a tiny batch with empty and absent parts (a follower without leaders or current clusters, no
    current cluster anywhere, no keep / sched), one about 100x larger, the tiny one again. Each step equals the
    checker, the third equals the first bit for bit; the timer reports KAD_ESTATE before the first call."""
    from kubeadmiral_amd import runtime
    c = runtime.Context(0)
    try:
        c.upload_snapshot(small_snapshot(3))
        with pytest.raises(runtime.KadError) as e:
            c.follower_timing()
        assert e.value.code == runtime.KAD_ESTATE
        rows = [[0, 1], [2], []]
        tiny = (FC.csr([[0, 1], [], [1, 2]]) + (np.zeros(4, np.int32), np.zeros(0, np.int32), np.array([0, 0, 1], np.uint8)))
        want = R.union_batch(tiny, [set(r) for r in rows])
        first = c.follower_union(3, tiny, leaders=FC.csr(rows))
        assert_equal(first, want)
        assert first["changed"].tolist() == [1, 0, 1] and first["count"].tolist() == [3, 0, 1]
        _assert_timing(c.follower_timing())
        lead, sets, fol, _ = FC.explicit_case(4100)
        assert len(lead[1]) >= 100 * 3  # leader ids: the tiny batch has 3
        assert_equal(c.follower_union(4100, fol, leaders=lead), R.union_batch(fol, sets))
        _assert_timing(c.follower_timing())
        again = c.follower_union(3, tiny, leaders=FC.csr(rows))
        assert_equal(again, want)
        for k in ("changed", "count", "out_off", "out_cluster"):
            assert again[k].tobytes() == first[k].tobytes(), k
        _assert_timing(c.follower_timing())
    finally:
        c.close()


def test_staging_buffer_resident_mode_small_large_small(ctx):
    """Resident mode on one context: without keep / sched (both parts absent) and no follower at all but one
    without leaders, then the full resident case, then the first again, bit for bit."""
    snap, fwk, batch, n_ids, L, keep, sched, fol = FC.resident_case()
    ctx.upload_snapshot(snap)
    res = ctx.run(fwk, batch)
    hdr = pack.header_of(batch.blob, pack.BatchHeader)
    cur_off = pack.array_of(batch.blob, hdr, pack.B_CUR_OFF, np.int32, hdr.n_units + 1)
    cur_id = pack.array_of(batch.blob, hdr, pack.B_CUR_ID, np.int32, int(cur_off[-1]))
    sets0 = R.resident_leader_sets(res.status, res.count, res.cluster, batch.out_off, cur_off, cur_id, L, None, None)
    tiny = (FC.csr([[0], [], [1, 0]]) + (np.zeros(4, np.int32), np.zeros(0, np.int32), np.zeros(3, np.uint8)))
    want = R.union_batch(tiny, sets0)
    first = ctx.follower_union(n_ids, tiny, n_leaders=L)
    assert_equal(first, want)
    _assert_timing(ctx.follower_timing())
    sets = R.resident_leader_sets(res.status, res.count, res.cluster, batch.out_off, cur_off, cur_id, L, sched, keep)
    assert_equal(ctx.follower_union(n_ids, fol, keep=keep, sched=sched, n_leaders=L), R.union_batch(fol, sets))
    _assert_timing(ctx.follower_timing())
    again = ctx.follower_union(n_ids, tiny, n_leaders=L)
    for k in ("changed", "count", "out_off", "out_cluster"):
        assert again[k].tobytes() == first[k].tobytes(), k
    _assert_timing(ctx.follower_timing())


def _pod_template(rng, w):
    spec = {"containers": [{"name": "c", "envFrom": [{"configMapRef": {"name": f"cm-{int(rng.integers(0, 40))}"}}],
                            "env": [{"name": "E", "valueFrom": {"secretKeyRef": {"name": f"sec-{int(rng.integers(0, 40))}", "key": "k"}}}]}],
            "volumes": [{"name": "v", "configMap": {"name": f"cm-{int(rng.integers(0, 40))}"}}]}
    if w % 3 == 0:
        spec["serviceAccountName"] = f"sa-{w % 6}"
    return {"metadata": {}, "spec": spec}


def _expected_followers(leaders, followers, s2f):
    """reconcileLeader + reconcileFollower, one object at a time, with the checker."""
    desired = {}
    for ld in leaders:
        ref = ("types.kubeadmiral.io", ld["kind"], ld["metadata"]["namespace"], ld["metadata"]["name"])
        for f in R.infer_followers(ld, ("apps", "Deployment"), s2f) or ():
            desired.setdefault(f, set()).add(ref)
    by_ref = {("types.kubeadmiral.io", ld["kind"], ld["metadata"]["namespace"], ld["metadata"]["name"]): ld for ld in leaders}
    out, needs = [], []
    for f in copy.deepcopy(followers):
        ref = ("types.kubeadmiral.io", f["kind"], f["metadata"]["namespace"], f["metadata"]["name"])
        want = desired.get(ref, set())
        cur = {(x.get("group", ""), x["kind"], x.get("namespace", ""), x["name"]) for x in f["spec"].get("follows") or []}
        leaders_changed = want != cur
        if leaders_changed:
            f["spec"]["follows"] = [dict(([("group", g)] if g else []) + [("kind", k)] + ([("namespace", ns)] if ns else []) +
                                         [("name", n)]) for g, k, ns, n in sorted(want)]
        union = set()
        for ld in want:
            for p in by_ref[ld]["spec"].get("placements") or []:
                union |= {c["name"] for c in p["placement"].get("clusters") or []}
        pls = f["spec"].get("placements") or []
        mine = next((p for p in pls if p["controller"] == "kubeadmiral.io/follower-controller"), None)
        cur_names = None if mine is None else [c["name"] for c in mine["placement"].get("clusters") or []]
        changed, after = R.set_placement_names(cur_names, union)
        if changed:
            pls = [p for p in pls if p is not mine]
            if after is not None:
                entry = {"controller": "kubeadmiral.io/follower-controller", "placement": {"clusters": [{"name": n} for n in after]}}
                pls = pls + [entry] if mine is None else [entry if p is mine else p for p in f["spec"]["placements"]]
            f["spec"]["placements"] = pls
        out.append(f)
        needs.append(leaders_changed or changed)
    return out, needs


def test_reconcile_followers_end_to_end(ctx):
    """~50 leaders, ~120 followers; resident == explicit == the checker applied object by object. Among the
    leaders: one whose policy is missing, objects whose Schedule fails (their unit has an error status: the
    placement they keep counts), objects whose apply fails although their unit is OK on the device (the
    unapplied result must not reach their followers), a sticky leader with a current cluster that left the
    snapshot, a leader with another controller's placement. Then a pass that schedules nothing."""
    from kubeadmiral_amd.controller import BatchReconciler

    rng = np.random.default_rng(31)
    ftc, clusters, objs, pols = synth.gen_trigger_workload(rng, 50, 16, n_policies=6)
    names = [c.name for c in clusters]
    by_key = {}
    for p in pols:
        if p.name not in ("policy-4", "policy-5"):
            p.spec.scheduling_mode = "Duplicate"     # every cluster that passes the filters is placed
        if p.spec.auto_migration is not None and p.name != "policy-4":
            p.spec.auto_migration.when.pod_unschedulable_for = "2m"   # policy-4 keeps nil: its objects' apply fails
        if p.name == "policy-5":
            p.spec.max_clusters = -1                                  # "failed to selectClusters"
        by_key[(p.namespace, p.name)] = p
    policy_of = [o["metadata"]["labels"][O.PROPAGATION_POLICY_NAME_LABEL] for o in objs]
    assert {"policy-4", "policy-5"} <= set(policy_of)
    old_placement = [{"controller": O.PREFIXED_GLOBAL_SCHEDULER_NAME,
                      "placement": {"clusters": [{"name": names[1]}, {"name": names[3]}]}}]
    for w, o in enumerate(objs):
        o["spec"]["template"]["spec"]["template"] = _pod_template(rng, w)
        if policy_of[w] in ("policy-4", "policy-5"):  # placed and enabled by an earlier pass; this one fails
            o["spec"]["placements"] = copy.deepcopy(old_placement)
            o["metadata"]["annotations"][O.ENABLE_FOLLOWER_SCHEDULING_ANNOTATION] = "true"
    plain = [w for w in range(len(objs)) if policy_of[w] not in ("policy-4", "policy-5")]
    missing, annotated, other, sticky = plain[:4]
    objs[missing]["metadata"]["labels"][O.PROPAGATION_POLICY_NAME_LABEL] = "missing"   # not scheduled: no followers wanted
    objs[annotated]["metadata"]["annotations"][FL.FOLLOWERS_ANNOTATION] = '[{"kind": "Service", "name": "svc-0"}]'
    objs[other]["spec"]["placements"] = [{"controller": "other-controller", "placement": {"clusters": [{"name": "left-the-fleet"}]}}]
    objs[sticky]["metadata"]["annotations"][O.STICKY_CLUSTER_ANNOTATION] = "true"
    objs[sticky]["spec"]["placements"] = [{"controller": O.PREFIXED_GLOBAL_SCHEDULER_NAME,
                                           "placement": {"clusters": [{"name": names[2]}, {"name": "left-the-fleet-2"}]}}]
    followers = []
    for kind, n in (("FederatedConfigMap", "cm"), ("FederatedSecret", "sec")):
        for k in range(55):
            f = {"apiVersion": "types.kubeadmiral.io/v1alpha1", "kind": kind,
                 "metadata": {"name": f"{n}-{k}", "namespace": "default"}, "spec": {"template": {}}}
            if k % 4 == 0:   # a stale placement and a stale leader
                f["spec"]["placements"] = [{"controller": FL.PREFIXED_CONTROLLER_NAME,
                                            "placement": {"clusters": [{"name": names[k % 16]}, {"name": "gone"}]}}]
                f["spec"]["follows"] = [{"group": "types.kubeadmiral.io", "kind": "FederatedDeployment", "namespace": "default", "name": "app-999"}]
            followers.append(f)
    for k in range(6):
        followers.append({"apiVersion": "types.kubeadmiral.io/v1alpha1", "kind": "FederatedServiceAccount",
                          "metadata": {"name": f"sa-{k}", "namespace": "default"}, "spec": {}})
    for kind, n in (("FederatedService", "svc-0"), ("FederatedService", "svc-unreferenced"),
                    ("FederatedIngress", "ing-0"), ("FederatedIngress", "ing-1")):
        followers.append({"apiVersion": "types.kubeadmiral.io/v1alpha1", "kind": kind,
                          "metadata": {"name": n, "namespace": "default"},
                          "spec": {"placements": [{"controller": FL.PREFIXED_CONTROLLER_NAME, "placement": {"clusters": [{"name": names[0]}]}}]}})
    assert len(followers) == 120

    rec = BatchReconciler(ftc, ctx=ctx)
    assert rec.last_pass is None                      # nothing reconciled yet
    outcomes = rec.reconcile(objs, by_key, clusters)
    stages = [o.stage for o in outcomes]
    assert stages.count("scheduled") >= 25 and "schedule-error" in stages and "apply-error" in stages
    assert stages[sticky] == "scheduled" and "left-the-fleet-2" in FL.placement_names(objs[sticky], O.PREFIXED_GLOBAL_SCHEDULER_NAME)
    for w, st in enumerate(stages):                   # the failed objects keep what they had
        if st in ("schedule-error", "apply-error"):
            assert objs[w]["spec"]["placements"] == old_placement, (w, st)
    units = rec.last_pass
    mapped = {i for i in units if i >= 0}
    assert mapped == {w for w, st in enumerate(stages) if st in ("scheduled", "schedule-error")}
    # the device does hold results that were never applied: OK units of the apply-error objects
    res = ctx.download()
    assert any(i < 0 and res.status[w] == 0 and res.count[w] > 0 for w, i in enumerate(units))
    assert any(i >= 0 and res.status[w] >= 3 for w, i in enumerate(units))
    assert any(i >= 0 and res.status[w] == 1 for w, i in enumerate(units))

    s2f = FL.default_source_to_federated()
    want, want_needs = _expected_followers(objs, followers, s2f)
    assert any(want_needs) and not all(want_needs)
    # some follower's union depends on a failed leader's kept placement alone
    explicit = copy.deepcopy(followers)
    needs_e, errors = rec.reconcile_followers(objs, explicit, clusters)
    assert not errors and needs_e == want_needs and explicit == want
    resident = copy.deepcopy(followers)
    needs_r, errors = rec.reconcile_followers(objs, resident, clusters, resident=units)
    assert not errors and needs_r == want_needs and resident == want
    # a second pass over the updated followers changes nothing
    needs_2, _ = rec.reconcile_followers(objs, resident, clusters, resident=units)
    assert not any(needs_2) and resident == want

    # a pass that schedules nothing (every trigger hash is unchanged): no unit of it is resident, so the
    # followers are reconciled from the dicts, whatever batch an earlier pass left on the device
    again = rec.reconcile(objs, by_key, clusters)
    assert all(o.stage in ("unchanged", "policy-not-found") for o in again), sorted({o.stage for o in again})
    assert rec.last_pass is None
    objs[plain[5]]["spec"]["placements"] = [{"controller": O.PREFIXED_GLOBAL_SCHEDULER_NAME,
                                              "placement": {"clusters": [{"name": names[7]}]}}]  # moved meanwhile
    want3, needs3 = _expected_followers(objs, resident, s2f)
    assert any(needs3)
    got3 = copy.deepcopy(resident)
    needs_g, errors = rec.reconcile_followers(objs, got3, clusters, resident=rec.last_pass)
    assert not errors and needs_g == needs3 and got3 == want3


def test_group_member_explicit_only(ctx):
    from kubeadmiral_amd import runtime
    lead, sets, fol, _ = FC.explicit_case(130)
    snap, fwk, batch, n_ids, L, keep, sched, rfol = FC.resident_case()
    ctx.upload_snapshot(snap)
    single = ctx.follower_union(130, fol, leaders=lead)
    g = runtime.GroupContext([0, 0])
    try:
        g.upload_snapshot(snap)
        g.upload_batch(batch)
        g.schedule(fwk)
        g.sync()
        m = g.member(1)
        got = m.follower_union(130, fol, leaders=lead)
        for k in ("changed", "count", "out_off", "out_cluster"):
            assert (got[k] == single[k]).all(), k
        with pytest.raises(runtime.KadError) as e:
            m.follower_union(n_ids, rfol, keep=keep, sched=sched, n_leaders=L)
        assert e.value.code == runtime.KAD_EUNSUPPORTED
    finally:
        g.close()
