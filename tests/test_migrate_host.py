"""Auto migration on the host: the reference's TestCountUnschedulablePods cases through automigration.py and
through the checker (migrate_ref.py), pod records, the capacity branches, DeepEqual, the annotation text and its
round trip through the scheduler's reader, the skip reasons, kad_migrate_estimate's argument validation
(kad_migrate_check, no GPU) and the launch decision."""
import json
import os

import numpy as np
import pytest

import migrate_cases as MC
import migrate_ref as R
from kubeadmiral_amd import automigration as AM
from kubeadmiral_amd import objects as O
from kubeadmiral_amd import runtime, synth

HERE = os.path.dirname(os.path.abspath(__file__))
with open(os.path.join(HERE, "golden", "automigration.json")) as _f:
    GOLDEN = json.load(_f)

SEC = 10**9
NOW = GOLDEN["now_ns"]
FTC = O.FederatedTypeConfig("apps", "v1", "Deployment", "deployments", "Namespaced", "spec.replicas",
                            "status.replicas", "status.readyReplicas")


@pytest.fixture(scope="module", autouse=True)
def library():
    from kubeadmiral_amd import build
    build.build()


def rfc3339(ns):
    import datetime
    t = datetime.datetime(1970, 1, 1) + datetime.timedelta(seconds=ns // SEC)
    return t.strftime("%Y-%m-%dT%H:%M:%S") + (f".{ns % SEC:09d}" if ns % SEC else "") + "Z"


def golden_pod(name):
    """newPod (util_test.go:99-122) as a pod dict."""
    p = GOLDEN["pods"][name]
    cond = {"type": "PodScheduled", "status": "True", "lastTransitionTime": rfc3339(NOW + p["transition_offset_ns"])}
    if not p["schedulable"]:
        cond.update(status="False", reason="Unschedulable")
    pod = {"kind": "pod", "apiVersion": "v1", "metadata": {}, "status": {"conditions": [cond]}}
    if p["terminating"]:
        pod["metadata"]["deletionTimestamp"] = rfc3339(NOW)
    return pod


@pytest.mark.parametrize("case", GOLDEN["cases"], ids=[c["cite"] for c in GOLDEN["cases"]])
def test_golden_count_unschedulable_pods(case):
    pods = [golden_pod(n) for n in case["pods"]]
    want = (case["count"], case["next_cross_in_ns"])
    assert AM.count_unschedulable_pods(pods, NOW, GOLDEN["threshold_ns"]) == want
    assert R.count_unschedulable([AM.pod_record(p) for p in pods], NOW, GOLDEN["threshold_ns"]) == want


def test_golden_expected_values():
    assert [c["count"] for c in GOLDEN["cases"]] == [0, 1, 0, 1, 2, 1]
    assert [c["next_cross_in_ns"] for c in GOLDEN["cases"]] == [None, None, 10 * SEC, 20 * SEC, 10 * SEC, 10 * SEC]


def _pod(conds, deleting=False):
    pod = {"metadata": {"name": "p"}, "status": {"conditions": conds}}
    if deleting:
        pod["metadata"]["deletionTimestamp"] = "2025-10-09T08:53:20Z"
    return pod


UNS = {"type": "PodScheduled", "status": "False", "reason": "Unschedulable", "lastTransitionTime": "2025-10-09T08:53:20Z"}
T0 = 1760000000 * SEC


def test_pod_record_variants():
    assert AM.parse_time("2025-10-09T08:53:20Z") == T0
    assert AM.pod_record(_pod([UNS])) == (AM.POD_UNSCHED, T0)
    assert AM.pod_record(_pod([])) == (0, 0)                                    # condition absent
    assert AM.pod_record({"metadata": {}}) == (0, 0)
    other = {"type": "Ready", "status": "False", "reason": "Unschedulable", "lastTransitionTime": "2025-10-09T08:53:20Z"}
    assert AM.pod_record(_pod([other])) == (0, 0)
    ok = dict(UNS, status="True")
    assert AM.pod_record(_pod([ok, UNS])) == (0, 0)                             # the second PodScheduled is ignored
    assert AM.pod_record(_pod([other, UNS, ok])) == (AM.POD_UNSCHED, T0)
    assert AM.pod_record(_pod([dict(UNS, status="True")])) == (0, 0)            # status "True"
    assert AM.pod_record(_pod([dict(UNS, reason="SchedulerError")])) == (0, 0)  # another reason
    assert AM.pod_record(_pod([dict(UNS, lastTransitionTime=None)])) == (AM.POD_UNSCHED | AM.POD_TZERO, 0)
    no_t = {k: v for k, v in UNS.items() if k != "lastTransitionTime"}
    assert AM.pod_record(_pod([no_t])) == (AM.POD_UNSCHED | AM.POD_TZERO, 0)
    assert AM.pod_record(_pod([dict(UNS, lastTransitionTime="0001-01-01T00:00:00Z")])) == (AM.POD_UNSCHED | AM.POD_TZERO, 0)
    assert AM.pod_record(_pod([UNS], deleting=True)) == (AM.POD_UNSCHED | AM.POD_DELETING, T0)
    # a zero-time pod always counts, whatever the threshold
    assert AM.count_unschedulable_pods([_pod([no_t])], T0, AM.TIME_MAX) == (1, None)
    assert R.count_unschedulable([AM.pod_record(_pod([no_t]))], T0, AM.TIME_MAX) == (1, None)


def test_parse_time():
    assert AM.parse_time("1970-01-01T00:00:00Z") == 0
    assert AM.parse_time("1970-01-01T01:00:00+01:00") == 0
    assert AM.parse_time("1969-12-31T23:59:59.5Z") == -SEC // 2
    assert AM.parse_time("2025-10-09T08:53:20.1234567891Z") == T0 + 123456789  # digits past the ninth are dropped
    assert AM.parse_time("2024-02-29T00:00:00Z") == 1709164800 * SEC
    assert AM.parse_time(None) is None
    for bad in ("2025-10-09 08:53:20Z", "2025-10-09T08:53:20", "2025-13-09T08:53:20Z", "2025-02-30T00:00:00Z", "", 5):
        with pytest.raises(O.ObjectError):
            AM.parse_time(bad)


def test_capacity_branches():
    assert AM.cluster_capacity(5, 5, 2) == 3       # n >= desired: the schedulable pods
    assert AM.cluster_capacity(7, 5, 3) == 4
    assert AM.cluster_capacity(3, 5, 2) == 3       # n < desired: uncreated pods count as schedulable
    assert AM.cluster_capacity(5, 5, 0) is None    # cap >= desired: no entry
    assert AM.cluster_capacity(9, 5, 2) is None
    assert AM.cluster_capacity(3, 5, 0) is None
    assert AM.cluster_capacity(3, 0, 3) is None    # desired 0: 0 >= 0
    assert AM.cluster_capacity(3, -2, 3) is None   # negative desired
    assert AM.cluster_capacity(0, 0, 0) is None
    for n, d, u in ((5, 5, 2), (3, 5, 2), (5, 5, 0), (3, 0, 3), (3, -2, 3)):
        recs = [(R.POD_UNSCHED, 0)] * u + [(0, 0)] * (n - u)
        assert R.estimate(100, 10, [(0, d, 0, recs)])[0][0][2] == AM.cluster_capacity(n, d, u)


def test_deep_equal_and_marshal():
    assert not AM.info_changed(None, {})                         # nil against empty
    assert not AM.info_changed({}, None)
    assert not AM.info_changed({"b": 1, "a": 2}, {"a": 2, "b": 1})
    assert AM.info_changed({"a": 2}, {"a": 2, "b": 1})           # an extra key
    assert AM.info_changed({"a": 2, "b": 1}, {"a": 2})           # a missing key
    assert AM.info_changed({"a": 2}, {"a": 3})                   # a differing value
    assert AM.decode_info("{not json") is None                    # invalid: as if absent
    assert AM.decode_info('{"estimatedCapacity":{"a":"x"}}') is None
    assert AM.decode_info('{"estimatedCapacity":null}') is None
    assert AM.decode_info("{}") is None
    assert AM.decode_info('{"estimatedCapacity":{"b":1,"a":2}}') == {"a": 2, "b": 1}
    assert AM.marshal_info({}) == "{}" and AM.marshal_info(None) == "{}"
    assert AM.marshal_info({"b": 1, "a": 0, "B": 7}) == '{"estimatedCapacity":{"B":7,"a":0,"b":1}}'


def _fed(annotations):
    return {"apiVersion": "types.kubeadmiral.io/v1alpha1", "kind": "FederatedDeployment",
            "metadata": {"name": "app", "namespace": "default", "annotations": dict(annotations)},
            "spec": {"template": {"apiVersion": "apps/v1", "kind": "Deployment", "metadata": {"name": "app", "namespace": "default"},
                                  "spec": {"replicas": 5}}}}


def _member(desired=5, total=5, ready=3):
    return {"apiVersion": "apps/v1", "kind": "Deployment", "spec": {"replicas": desired},
            "status": {"replicas": total, "readyReplicas": ready}}


def _uns_pods(n_crossed, n_ok, in_10s=0):
    crossed = dict(UNS, lastTransitionTime=rfc3339(T0 - 120 * SEC))
    soon = dict(UNS, lastTransitionTime=rfc3339(T0 - 50 * SEC))
    ok = {"type": "PodScheduled", "status": "True", "lastTransitionTime": rfc3339(T0 - 500 * SEC)}
    return [_pod([crossed])] * n_crossed + [_pod([ok])] * n_ok + [_pod([soon])] * in_10s


def test_reconcile_object_and_round_trip():
    obj = _fed({O.POD_UNSCHEDULABLE_THRESHOLD_ANNOTATION: "1m0s", O.AUTO_MIGRATION_INFO_ANNOTATION: "{broken"})
    cobjs = [("c-b", _member()), ("c-a", _member(desired=4, total=4, ready=1)), ("c-ready", _member(ready=5))]
    pods = [_uns_pods(2, 3), _uns_pods(3, 1, in_10s=1), _uns_pods(5, 0)]
    result, caps, updated = AM.reconcile_object(FTC, obj, cobjs, pods, T0)
    assert caps == {"c-b": 3, "c-a": 2} and result == (10 * SEC, False) and updated
    text = obj["metadata"]["annotations"][O.AUTO_MIGRATION_INFO_ANNOTATION]
    assert text == '{"estimatedCapacity":{"c-a":2,"c-b":3}}'
    # the scheduler reads the same EstimatedCapacity back
    pol = O.PropagationPolicy("p", "default", 1, O.PropagationPolicySpec(auto_migration=O.AutoMigration()))
    su = O.scheduling_unit_for_fed_object(FTC, obj, pol)
    assert su.auto_migration.estimated_capacity == caps
    # a second reconcile finds nothing to write
    assert AM.reconcile_object(FTC, obj, cobjs, pods, T0) == (result, caps, False)
    # no capacity short of desired: {} is written over a non-empty annotation, and left alone after that
    calm = [_uns_pods(0, 5), _uns_pods(0, 4), []]
    assert AM.reconcile_object(FTC, obj, cobjs, calm, T0) == (None, {}, True)
    assert obj["metadata"]["annotations"][O.AUTO_MIGRATION_INFO_ANNOTATION] == "{}"
    assert AM.reconcile_object(FTC, obj, cobjs, calm, T0) == (None, {}, False)


def test_disabled_case_deletes_annotation():
    for ann in ({}, {O.POD_UNSCHEDULABLE_THRESHOLD_ANNOTATION: "soon"}):
        obj = _fed(dict(ann, **{O.AUTO_MIGRATION_INFO_ANNOTATION: '{"estimatedCapacity":{"c":1}}', "keep": "me"}))
        assert AM.reconcile_object(FTC, obj, [("c", _member())], [_uns_pods(2, 3)], T0) == (None, None, True)
        assert O.AUTO_MIGRATION_INFO_ANNOTATION not in obj["metadata"]["annotations"]
        assert obj["metadata"]["annotations"]["keep"] == "me"
        assert AM.reconcile_object(FTC, obj, [("c", _member())], [_uns_pods(2, 3)], T0) == (None, None, False)


def test_skip_reasons_and_backoff():
    live = _uns_pods(2, 3)
    assert AM.segment_of(FTC, _member(), live) == (0, 5)
    assert AM.segment_of(FTC, _member(total=5, ready=5), live) == (AM.SEG_SKIP, 0)           # total == ready
    no_status = {"spec": {"replicas": 5}}
    assert AM.segment_of(FTC, no_status, live) == (AM.SEG_SKIP, 0)                            # both default to 0
    bad_status = {"spec": {"replicas": 5}, "status": {"replicas": "5", "readyReplicas": 5}}
    assert AM.segment_of(FTC, bad_status, live) == (0, 5)                                     # an error does not skip
    assert AM.segment_of(FTC, {"status": {"replicas": 5, "readyReplicas": 1}}, live) == (AM.SEG_SKIP, 0)  # no desired
    assert AM.segment_of(FTC, {"spec": {"replicas": 1.5}, "status": {"replicas": 5}}, live) == (AM.SEG_SKIP, 0)
    assert AM.segment_of(FTC, _member(), AM.PodListError("x")) == (AM.SEG_SKIP | AM.SEG_BACKOFF, 5)
    assert AM.segment_of(FTC, _member(), AM.PodListError("no plugin", needs_backoff=False)) == (AM.SEG_SKIP, 5)
    caps, result = AM.estimate_capacity(FTC, [("a", _member()), ("b", _member())], [AM.PodListError("x"), live], T0, 60 * SEC)
    assert caps == {"b": 3} and result == (None, True)
    caps, result = AM.estimate_capacity(FTC, [("a", _member(ready=5))], [live], T0, 60 * SEC)
    assert caps == {} and result is None


def test_packer_matches_host_path_and_checker():
    """MigrationBatch's arrays through the checker and through migrate_numpy == the per-object host path."""
    a, stale = synth.gen_migration(3, 60, 20, ready_share=0.4, extra_ids=2, changed=0.3)
    names = [f"cluster-{i:02d}" for i in range(22)]
    ftc, objs, cobjs, pods = synth.migration_objects(a, names)
    batch = AM.MigrationBatch(ftc, names[:20], a["now_ns"])
    for o, c, p in zip(objs, cobjs, pods):
        batch.add(o, AM.threshold_of(o), c, p)
    arr = batch.arrays()
    assert runtime.migrate_check(20, **arr) == 0
    want = R.run(**arr)
    got = AM.migrate_numpy(**arr)
    for k in want:
        assert [int(x) for x in got[k]] == want[k], k
    assert [bool(x) for x in want["changed"]] == [bool(x) for x in stale]
    for i, (o, c, p) in enumerate(zip(objs, cobjs, pods)):
        result, caps, updated = AM.reconcile_object(ftc, o, c, p, a["now_ns"])
        assert caps == batch.capacities(got, i) and result == batch.result(got, i) and updated == bool(got["changed"][i])
    with pytest.raises(ValueError):
        batch.add(objs[0], 1, [("x", {}), ("x", {})], [[], []])


def _check(arr, C=MC.N_IDS, **change):
    a = dict(arr)
    for k, v in change.items():
        a[k] = v if not callable(v) else v(np.array(a[k]))
    return runtime.migrate_check(C, **a)


def test_migrate_check_rejects():
    arr, _ = MC.shapes_case(16)
    assert _check(arr) == 0
    assert _check(arr, C=MC.N_IDS + 1) == runtime.KAD_EINVAL          # n_ids below the snapshot's clusters
    assert _check(arr, n_ids=131073, C=0) == runtime.KAD_EINVAL

    def at(i, v):
        def f(x):
            x[i] = v
            return x
        return f

    def bump(i, d):
        def f(x):
            x[i] += d
            return x
        return f
    # non-monotone offsets, offsets that do not start at 0 or do not end at their count
    assert _check(arr, obj_seg_off=at(3, 0)) == runtime.KAD_EINVAL
    assert _check(arr, seg_pod_off=at(10, 0)) == runtime.KAD_EINVAL
    assert _check(arr, old_off=at(2, int(arr["old_off"][-1]) + 5)) == runtime.KAD_EINVAL
    assert _check(arr, obj_seg_off=at(0, 1)) == runtime.KAD_EINVAL
    assert _check(arr, seg_pod_off=bump(-1, 1)) == runtime.KAD_EINVAL
    assert _check(arr, seg_pod_off=bump(-1, -1)) == runtime.KAD_EINVAL
    assert _check(arr, obj_seg_off=bump(-1, -1)) == runtime.KAD_EINVAL
    assert _check(arr, old_off=bump(-1, 1)) == runtime.KAD_EINVAL
    # ids out of range
    assert _check(arr, seg_cluster=at(0, MC.N_IDS)) == runtime.KAD_EINVAL
    assert _check(arr, seg_cluster=at(0, -1)) == runtime.KAD_EINVAL
    assert _check(arr, old_cluster=at(0, MC.N_IDS)) == runtime.KAD_EINVAL
    assert _check(arr, old_cluster=at(0, -1)) == runtime.KAD_EINVAL
    assert _check(arr, old_off=at(0, 1)) == runtime.KAD_EINVAL          # old_off not from 0 (its twin: arr itself)
    # descending or duplicate clusters within an object (the last object has four ascending segments)
    so = arr["obj_seg_off"]
    o = max(i for i in range(len(so) - 1) if so[i + 1] - so[i] >= 2)
    s = int(so[o])
    assert _check(arr, seg_cluster=at(s + 1, int(arr["seg_cluster"][s]))) == runtime.KAD_EINVAL
    assert _check(arr, seg_cluster=at(s, int(arr["seg_cluster"][s + 1]) + 1)) == runtime.KAD_EINVAL
    oo = arr["old_off"]
    q = int(oo[max(i for i in range(len(oo) - 1) if oo[i + 1] - oo[i] >= 2)])
    assert _check(arr, old_cluster=at(q + 1, int(arr["old_cluster"][q]))) == runtime.KAD_EINVAL
    # the time domain
    assert _check(arr, now_ns=-1) == runtime.KAD_EINVAL
    assert _check(arr, now_ns=MC.TMAX + 1) == runtime.KAD_EINVAL
    assert _check(arr, now_ns=MC.TMAX) == 0 and _check(arr, now_ns=0) == 0
    live = int(np.nonzero((arr["pod_flags"] & R.POD_TZERO) == 0)[0][0])
    assert _check(arr, pod_t_ns=at(live, MC.TMAX + 1)) == runtime.KAD_EINVAL
    assert _check(arr, pod_t_ns=at(live, -MC.TMAX - 1)) == runtime.KAD_EINVAL
    assert _check(arr, pod_t_ns=at(live, -MC.TMAX)) == 0
    zero = int(np.nonzero(arr["pod_flags"] & R.POD_TZERO)[0][0])
    assert _check(arr, pod_t_ns=at(zero, MC.TMAX + 1)) == 0            # not read under POD_TZERO
    assert _check(arr, obj_threshold_ns=at(0, MC.TMAX + 1)) == runtime.KAD_EINVAL
    assert _check(arr, obj_threshold_ns=at(0, -MC.TMAX - 1)) == runtime.KAD_EINVAL
    # flags
    assert _check(arr, pod_flags=at(0, 8)) == runtime.KAD_EINVAL
    assert _check(arr, seg_flags=at(0, 4)) == runtime.KAD_EINVAL
    assert _check(arr, seg_flags=at(0, R.SEG_BACKOFF)) == runtime.KAD_EINVAL
    for edge_now in (0, MC.TMAX):
        assert runtime.migrate_check(MC.N_IDS, **MC.edge_case(edge_now)) == 0


def test_route_migrate_boundaries():
    ev = runtime.migrate_route_eval
    r = ev(1000, 8000, 0, 300)
    assert r["threads"] == 256 and r["long_min"] >= 64 and r["long_grid"] == 0
    # the group width: the mean segment length rounded up to a power of two, within [8, 64]
    for pods, width in ((0, 8), (1000, 8), (8000, 8), (8001, 16), (16000, 16), (16001, 32), (32000, 32), (32001, 64),
                        (64000, 64), (10**9, 64)):
        assert ev(1000, pods, 0, 300)["width"] == width, pods
    for segs, ow in ((0, 8), (2400, 8), (2401, 16), (4801, 32), (9601, 64), (10**6, 64)):
        assert ev(segs, 0, 0, 300)["obj_width"] == ow, segs
    # the grids: one lane group per segment / object until 8 blocks a CU are reached, then the groups stride
    for w_pods, per in ((8, 32), (16, 16), (32, 8), (64, 4)):
        for S in (1, per, per + 1, 100 * per):
            r = ev(S, S * w_pods, 0, 1, n_cu=256)
            assert r["width"] == w_pods and r["grid"] == (S + per - 1) // per and r["stride"] == r["grid"] * per
    r = ev(10**6, 8 * 10**6, 7, 10**6, n_cu=4)
    assert r["grid"] == 32 and r["stride"] == 32 * 32 and r["long_grid"] == 7 and r["obj_grid"] == 32
    assert ev(0, 0, 0, 0)["grid"] == 0 and ev(0, 0, 0, 0)["obj_grid"] == 0
    assert ev(0, 0, 0, 5)["obj_grid"] == 1
    lib = runtime.load_library()
    out = (runtime.ctypes.c_int32 * len(runtime.MIGRATE_ROUTE))()
    for bad in ((-1, 0, 0, 0, 1), (1, -1, 0, 0, 1), (1, 1, 2, 0, 1), (1, 1, 0, -1, 1), (1, 1, 0, 0, 0)):
        assert lib.kad_migrate_route_eval(*bad, out) == runtime.KAD_EINVAL
    assert {"kad_migrate_estimate", "kad_migrate_check", "kad_migrate_timing", "kad_migrate_route_eval",
            "kad_migrate_last_route"} <= set(runtime.declared_functions())
