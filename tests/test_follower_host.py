"""Follower scheduling on the host: inference against the reference's tables through follower.py and through
the checker (follower_ref.py), the controller's caches, the CSR, kad_follower_union's argument validation
(kad_follower_check, no GPU), the launch decision and the capacity protocol of Context.follower_union."""
import ctypes
import json
import os

import numpy as np
import pytest

import follower_cases as FC
import follower_ref as R
from kubeadmiral_amd import follower as FL
from kubeadmiral_amd import objects as O
from kubeadmiral_amd import runtime

HERE = os.path.dirname(os.path.abspath(__file__))
with open(os.path.join(HERE, "golden", "follower.json")) as _f:
    GOLDEN = json.load(_f)


@pytest.fixture(scope="module", autouse=True)
def library():
    from kubeadmiral_amd import build
    build.build()


def _leader(spec, annotations=None, enabled=True, kind=("apps/v1", "Deployment"), path=("template",)):
    ann = dict(annotations or {})
    if enabled:
        ann[O.ENABLE_FOLLOWER_SCHEDULING_ANNOTATION] = "true"
    inner = {"spec": spec}
    for p in reversed(path):
        inner = {p: inner}
    tmpl = {"apiVersion": kind[0], "kind": kind[1], "spec": inner} if path else {"apiVersion": kind[0], "kind": kind[1], "spec": spec}
    return {"apiVersion": "types.kubeadmiral.io/v1alpha1", "kind": "Federated" + kind[1],
            "metadata": {"name": "leader", "namespace": "default", "annotations": ann}, "spec": {"template": tmpl}}


def test_golden_followers_from_pod():
    g = GOLDEN["TestGetFollowersFromPod"]
    s2f = {tuple(k): tuple(v) for k, v in g["sourceToFederatedGKMap"]}
    want = {(gk[0], gk[1], g["namespace"], n) for gk, names in g["expectedNamesByGK"] for n in names}
    assert len(want) == 8 + 19 + 1 + 1
    assert R.followers_from_pod(g["namespace"], g["podSpec"], s2f) == want
    assert {tuple(f) for f in FL.followers_from_pod(g["namespace"], g["podSpec"], s2f)} == want
    # through inferFollowers, for every leader type's pod template path
    for gk, path in FL.LEADER_POD_TEMPLATE_PATHS.items():
        api = f"{gk[0]}/v1" if gk[0] else "v1"
        obj = _leader(g["podSpec"], kind=(api, gk[1]), path=tuple(path.split(".")[1:]))
        assert FL.source_group_kind(obj) == gk
        # getPodSpec decodes what it finds at the path as a PodTemplateSpec and returns its .spec
        # (util.go:165-169): at a Pod's path "spec" that is the pod spec itself, which has no "spec" field
        expect = want if gk != ("", "Pod") else set()
        assert {tuple(f) for f in FL.infer_followers(obj, gk, s2f)} == expect, gk
        assert R.infer_followers(obj, gk, s2f) == expect, gk


@pytest.mark.parametrize("table,fn,ref", [("TestPodSecrets", FL.pod_secret_names, R.secret_names),
                                          ("TestPodConfigmaps", FL.pod_configmap_names, R.configmap_names)])
def test_golden_name_tables(table, fn, ref):
    g = GOLDEN[table]
    assert fn(g["podSpec"]) == set(g["expectedNames"]) == ref(g["podSpec"])
    assert fn(g["emptyPodSpec"]) == set() == ref(g["emptyPodSpec"])


def test_first_volume_source_wins():
    """The visitors switch over the volume sources: a volume with two of them set yields the first case only."""
    spec = {"volumes": [{"secret": {"secretName": "late"}, "azureFile": {"secretName": "early"}},
                        {"configMap": {"name": "late"}, "projected": {"sources": [{"configMap": {"name": "early"}}]}}]}
    assert FL.pod_secret_names(spec) == {"early"} == R.secret_names(spec)
    assert FL.pod_configmap_names(spec) == {"early"} == R.configmap_names(spec)


def test_annotation_gate_and_errors():
    s2f = FL.default_source_to_federated()
    gk = ("apps", "Deployment")
    spec = {"containers": [{"envFrom": [{"configMapRef": {"name": "cm"}}]}]}
    for obj in (_leader(spec, enabled=False), _leader(spec, {O.ENABLE_FOLLOWER_SCHEDULING_ANNOTATION: "True"}, enabled=False)):
        assert FL.infer_followers(obj, gk, s2f) is None and R.infer_followers(obj, gk, s2f) is None
    ann = {FL.FOLLOWERS_ANNOTATION: json.dumps([{"kind": "Service", "name": "svc"},
                                                {"group": "networking.k8s.io", "kind": "Ingress", "name": "ing"}])}
    want = {("types.kubeadmiral.io", "FederatedConfigMap", "default", "cm"),
            ("types.kubeadmiral.io", "FederatedService", "default", "svc"),
            ("types.kubeadmiral.io", "FederatedIngress", "default", "ing")}
    obj = _leader(spec, ann)
    assert {tuple(f) for f in FL.infer_followers(obj, gk, s2f)} == want == R.infer_followers(obj, gk, s2f)
    # an unknown source type, and an annotation that is not JSON: the reference's errors
    for bad in (json.dumps([{"kind": "Gadget", "name": "x"}]), "{not json"):
        obj = _leader(spec, {FL.FOLLOWERS_ANNOTATION: bad})
        with pytest.raises(FL.FollowerError) as e:
            FL.infer_followers(obj, gk, s2f)
        with pytest.raises(R.RefError):
            R.infer_followers(obj, gk, s2f)
        if "Gadget" in bad:
            assert "no federated type config found for source type Gadget" in str(e.value)
    # no pod template at the leader type's path
    obj = _leader(spec)
    del obj["spec"]["template"]["spec"]["template"]
    with pytest.raises(FL.FollowerError, match="pod template does not exist"):
        FL.infer_followers(obj, gk, s2f)
    with pytest.raises(R.RefError):
        R.infer_followers(obj, gk, s2f)


def test_follower_index():
    ix = FL.FollowerIndex()
    a, b = FL.LeaderReference("g", "FederatedDeployment", "ns", "a"), FL.LeaderReference("g", "FederatedDeployment", "ns", "b")
    cm = FL.FollowerReference("g", "FederatedConfigMap", "ns", "cm")
    sec = FL.FollowerReference("g", "FederatedSecret", "ns", "sec")
    assert ix.update_leader(a, {cm, sec}) == {cm, sec}
    assert ix.update_leader(b, {cm}) == {cm}
    assert ix.desired_leaders(cm) == {a, b} and ix.desired_leaders(sec) == {a}
    # the follower object still lists a leader that dropped it: that follower is re-enqueued with the leader
    obj = {"spec": {"follows": [a.to_json(), b.to_json()]}}
    assert ix.observe_follower(cm, obj) == {a, b} and not ix.leaders_changed(cm, obj)
    assert ix.update_leader(b, {sec}) == {sec, cm}
    assert ix.desired_leaders(cm) == {a} and ix.leaders_changed(cm, obj)
    assert ix.desired_leaders(sec) == {a, b}
    # a deleted leader (or one with follower scheduling off) wants no followers
    assert ix.update_leader(a, None) == {cm}
    assert ix.desired_leaders(cm) == set() and ix.desired_leaders(sec) == {b}
    assert a not in ix.from_leaders.cache and cm not in ix.from_leaders.reverse
    ix.observe_follower(cm, None)
    assert ix.from_followers.reverse_lookup(a) == set()
    # nil and empty are equal
    assert not ix.leaders_changed(cm, {"spec": {}}) and not ix.leaders_changed(cm, {"spec": {"follows": []}})


def test_csr_construction():
    ix = FL.FollowerIndex()
    ld = [FL.LeaderReference("g", "K", "ns", n) for n in "abc"]
    f = [FL.FollowerReference("g", "FederatedConfigMap", "ns", n) for n in ("x", "y", "z")]
    ix.update_leader(ld[0], {f[0], f[1]})
    ix.update_leader(ld[1], {f[1]})
    ix.update_leader(ld[2], {f[1]})
    off, idx, lists = ix.csr(f, {ld[0]: 5, ld[1]: 3})  # leader c is absent from the caller's list
    assert off.tolist() == [0, 1, 4, 4] and off.dtype == np.int32 and idx.dtype == np.int32
    assert idx.tolist() == [5, 5, 3, -1] and lists[1] == sorted(ld) and lists[2] == []


def test_set_placement_names_and_apply_helpers():
    obj = {"spec": {"placements": [{"controller": "other", "placement": {"clusters": [{"name": "z"}]}},
                                    {"controller": FL.PREFIXED_CONTROLLER_NAME, "placement": {"clusters": [{"name": "b"}, {"name": "a"}]}}]}}
    assert FL.placement_names(obj, FL.PREFIXED_CONTROLLER_NAME) == ["b", "a"]
    assert FL.placement_names(obj, "none") is None
    assert sorted(FL.placement_names(obj)) == ["a", "b", "z"]
    assert FL.placement_names(obj, None, exclude="other") == ["b", "a"]
    assert R.set_placement_names(["b", "a", "a"], {"a", "b"}) == (False, ["b", "a", "a"])
    assert R.set_placement_names(["b"], {"a", "b"}) == (True, ["a", "b"])
    assert R.set_placement_names([], set()) == (True, None) and R.set_placement_names(None, set()) == (False, None)
    assert R.leader_placement_union([0, -1, 2, 0], [{1}, {2}, None]) == {1}
    FL.set_follows(obj, [FL.LeaderReference("", "K", "", "n"), FL.LeaderReference("g", "K", "ns", "a")])
    assert obj["spec"]["follows"] == [{"kind": "K", "name": "n"}, {"group": "g", "kind": "K", "namespace": "ns", "name": "a"}]


# ------------------------------------------------------------------ kad_follower_check (no GPU)
def _check(C, W, n_ids, fol, **kw):
    return runtime.follower_check(C, W, n_ids, fol, **kw)


def _fol(fol=((0,),), cur=((),), has=(0,)):
    fo, fl = FC.csr([list(x) for x in fol])
    co, cc = FC.csr([list(x) for x in cur])
    return fo, fl, co, cc, np.array(has, np.uint8)


def test_abi_validation_without_gpu():
    EINVAL, ESTATE = runtime.KAD_EINVAL, runtime.KAD_ESTATE
    lead = FC.csr([[0, 1], [2]])
    assert _check(3, -1, 3, _fol(), leaders=lead) == 0
    assert _check(3, -1, 131072, _fol(), leaders=lead) == 0
    assert _check(3, -1, 2, _fol(), leaders=FC.csr([[0], [1]])) == EINVAL        # n_ids < C
    assert _check(3, -1, 131073, _fol(), leaders=lead) == EINVAL                  # n_ids > 131072
    assert _check(3, -1, 3, _fol(), leaders=FC.csr([[0, 3], [2]])) == EINVAL      # id >= n_ids
    assert _check(3, -1, 3, _fol(), leaders=FC.csr([[0, -1], [2]])) == EINVAL     # -1 is not an id here
    assert _check(3, -1, 3, _fol(fol=((2,),)), leaders=lead) == EINVAL            # leader index >= n_leaders
    assert _check(3, -1, 3, _fol(fol=((-2,),)), leaders=lead) == EINVAL
    assert _check(3, -1, 3, _fol(fol=((-1,),)), leaders=lead) == 0
    assert _check(3, -1, 3, _fol(cur=((3,),), has=(1,)), leaders=lead) == EINVAL  # current id out of range
    for which in ("leaders", "keep"):                                            # offsets: not from 0, not monotone
        for off in ([1, 2, 3], [0, 2, 1]):
            bad = (np.array(off, np.int32), np.array([0, 1, 2], np.int32))
            kw = {"leaders": lead, which: bad}
            assert _check(3, -1, 3, _fol(), **kw) == EINVAL, (which, off)
    f = list(_fol(fol=((0,), (1,)), cur=((), ()), has=(0, 0)))
    f[0] = np.array([0, 2, 1], np.int32)
    assert _check(3, -1, 3, tuple(f), leaders=lead) == EINVAL                     # fol_off not monotone
    f = list(_fol(fol=((0,), (1,)), cur=((0,), (1,)), has=(1, 1)))
    f[2] = np.array([0, 2, 1], np.int32)
    assert _check(3, -1, 3, tuple(f), leaders=lead) == EINVAL                     # cur_off not monotone
    assert _check(3, -1, 3, _fol(), leaders=lead, capacity=-1) == EINVAL
    # an entry that does not exist holds no clusters; an entry that exists may be empty
    assert _check(3, -1, 3, _fol(cur=((1,),), has=(0,)), leaders=lead) == EINVAL
    assert _check(3, -1, 3, _fol(cur=((),), has=(1,)), leaders=lead) == 0
    # resident mode: needs a scheduled batch; n_leaders >= its units; sched ids and offsets checked
    assert _check(3, -1, 3, _fol(), n_leaders=2) == ESTATE
    assert _check(3, 2, 3, _fol(), n_leaders=2) == 0
    assert _check(3, 2, 3, _fol(), n_leaders=1) == EINVAL
    assert _check(3, 2, 3, _fol(), n_leaders=2, sched=FC.csr([[0], [2]])) == 0
    assert _check(3, 2, 3, _fol(), n_leaders=2, sched=FC.csr([[0], [3]])) == EINVAL
    assert _check(3, 2, 3, _fol(), n_leaders=3, keep=FC.csr([[0], [2], [1]])) == 0
    assert _check(3, 2, 3, _fol(fol=((2,),)), n_leaders=3, keep=FC.csr([[0], [2], [1]])) == 0
    # one malformed CSR per array the cases above leave out, each beside its well-formed twin
    assert _check(3, -1, 3, _fol(), leaders=lead, keep=FC.csr([[0], [2]])) == 0
    assert _check(3, -1, 3, _fol(), leaders=lead, keep=FC.csr([[0], [3]])) == EINVAL     # keep id >= n_ids
    assert _check(3, -1, 3, _fol(), leaders=lead, keep=FC.csr([[-1], [2]])) == EINVAL    # keep id < 0
    for off in ([1, 1, 2], [0, 2, 1]):                                               # sched_off: start, monotone
        bad = (np.array(off, np.int32), np.array([0, 2], np.int32))
        assert _check(3, 2, 3, _fol(), n_leaders=2, sched=bad) == EINVAL, off
    for i in (0, 2):                                                                 # fol_off / cur_off from 1
        f = list(_fol(fol=((0,), (1,)), cur=((0,), (1,)), has=(1, 1)))
        assert _check(3, -1, 3, tuple(f), leaders=lead) == 0
        f[i] = np.array([1, 1, 2], np.int32)
        assert _check(3, -1, 3, tuple(f), leaders=lead) == EINVAL, i


def test_follower_route_eval():
    for n_ids in FC.N_IDS:
        r = runtime.follower_route_eval(n_ids, 100000)
        assert r["path"] == ("WAVE" if n_ids <= 8192 else "BLOCK") and r["words"] == (n_ids + 31) // 32, n_ids
        assert r["threads"] == 256 and 0 < r["grid"] and r["lds"] <= 65536
        assert r["stride"] == r["grid"] * (4 if r["path"] == "WAVE" else 1)
    assert runtime.follower_route_eval(8192, 10)["grid"] == 3 and runtime.follower_route_eval(8193, 10)["grid"] == 10
    assert runtime.follower_route_eval(100, 0)["grid"] == 0
    with pytest.raises(ValueError):
        runtime.follower_route_eval(131073, 1)


class _FakeLib:
    """kad_follower_union's capacity protocol without a device: the union of every follower is {0, 1, 2}."""

    def __init__(self):
        self.capacities = []

    def kad_follower_union(self, h, b, v):
        b, v = b._obj, v._obj
        F = b.n_followers
        self.capacities.append(b.out_capacity)
        off = np.ctypeslib.as_array(ctypes.cast(v.out_off, ctypes.POINTER(ctypes.c_int64)), (F + 1,))
        off[:] = 3 * np.arange(F + 1)
        np.ctypeslib.as_array(ctypes.cast(v.changed, ctypes.POINTER(ctypes.c_uint8)), (F,))[:] = 1
        np.ctypeslib.as_array(ctypes.cast(v.count, ctypes.POINTER(ctypes.c_int32)), (F,))[:] = 3
        if b.out_capacity < 3 * F:
            return runtime.KAD_ENOSPC
        np.ctypeslib.as_array(ctypes.cast(v.out_cluster, ctypes.POINTER(ctypes.c_int32)), (3 * F,))[:] = np.tile([0, 1, 2], F)
        return 0

    def kad_last_error(self, h):
        return b"out_capacity too small"


def test_capacity_protocol():
    ctx = runtime.Context.__new__(runtime.Context)
    ctx.h, ctx.L = None, _FakeLib()
    fol = _fol(fol=((0,), (0,), (0,)), cur=((), (), ()), has=(0, 0, 0))
    lead = FC.csr([[0, 1, 2]])
    r = ctx.follower_union(3, fol, leaders=lead, capacity=4)
    assert ctx.L.capacities == [4, 9] and r["calls"] == 2          # the retry asks for out_off[F] slots
    assert r["out_off"].tolist() == [0, 3, 6, 9] and r["out_cluster"].tolist() == [0, 1, 2] * 3
    ctx.L = _FakeLib()
    assert ctx.follower_union(3, fol, leaders=lead, capacity=9)["calls"] == 1
    ctx.L = _FakeLib()
    with pytest.raises(runtime.KadError) as e:
        ctx.follower_union(3, fol, leaders=lead, capacity=4, retry=False)
    assert e.value.code == runtime.KAD_ENOSPC and e.value.partial["out_off"].tolist() == [0, 3, 6, 9]
    assert e.value.partial["count"].tolist() == [3, 3, 3]


def test_resident_batch_holds_every_status_class():
    """On the C oracle alone: the batch the GPU resident-mode test schedules contains OK, sticky, no-feasible
    and error-status units, and an OK unit with clusters, a sticky unit with current clusters."""
    from gpu_util import c_oracle
    snap, fwk, batch, *_ = FC.resident_case()
    want = c_oracle(snap, batch, fwk)
    assert all(FC.status_classes(want.status).values()), FC.status_classes(want.status)
    assert (want.count[want.status == 0] > 0).any()
    from kubeadmiral_amd import pack
    hdr = pack.header_of(batch.blob, pack.BatchHeader)
    cur_off = pack.array_of(batch.blob, hdr, pack.B_CUR_OFF, np.int32, hdr.n_units + 1)
    assert (np.diff(cur_off)[want.status == 1] > 0).any()


def test_checker_sees_every_shape():
    for n_ids in FC.N_IDS:
        _, sets, fol, shapes = FC.explicit_case(n_ids)
        changed, count, off, out = R.union_batch(fol, sets)
        assert changed[shapes["delete"]] == 1 and count[shapes["delete"]] == 0
        assert changed[shapes["delete-empty-entry"]] == 1
        assert changed[shapes["nothing"]] == 0 and changed[shapes["only-absent"]] == 0
        assert changed[shapes["same-set-other-order"]] == 0 and count[shapes["same-set-other-order"]] > 0
        assert changed[shapes["leaders-65-same"]] == 0
        if n_ids > 65:
            assert changed[shapes["leaders-65"]] == 1 and changed[shapes["leader-twice"]] == 1
        assert off[-1] == len(out) == int(count[changed == 1].sum())


def test_last_pass_follows_the_outcomes():
    """BatchReconciler.last_pass names, per resident unit, the object that unit's device result describes: only
    objects whose result was applied or whose Schedule failed; None when the pass scheduled nothing."""
    from kubeadmiral_amd.controller import BatchReconciler, ReconcileOutcome

    rec = BatchReconciler.__new__(BatchReconciler)
    rec._pass = None
    assert rec.last_pass is None
    out = [None] * 6
    rec._record_pass(4, [(5, 0), (2, 1), (3, 2), (0, 3)], out)
    assert rec.last_pass == [-1, -1, -1, -1]      # nothing applied yet
    out[5] = ReconcileOutcome("AllOK", "scheduled", True)
    out[2] = ReconcileOutcome("Error", "apply-error")
    out[3] = ReconcileOutcome("Error", "schedule-error")
    out[0] = ReconcileOutcome("Error", "unit-error")
    assert rec.last_pass == [5, -1, 3, -1]
