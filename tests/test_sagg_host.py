"""Status aggregation on the host: statusagg.py against the reference's own table (tests/golden/
statusaggregator.json, TestJobPlugin) and the independent checker (sagg_ref.py), every branch of the two plugins
and of IsResourcePropagated, kad_sagg_check's rules and the route's boundaries. No GPU."""
import copy
import json
import os

import numpy as np
import pytest

import sagg_cases as SC
import sagg_ref as R
from kubeadmiral_amd import runtime, synth
from kubeadmiral_amd import statusagg as SA

HERE = os.path.dirname(os.path.abspath(__file__))
with open(os.path.join(HERE, "golden", "statusaggregator.json")) as f:
    GOLDEN = json.load(f)
NOW = 1_704_067_300


@pytest.fixture(scope="module", autouse=True)
def library():
    from kubeadmiral_amd import build
    build.build()


def through_batch(kind, source, fed, objs, now=NOW):
    """One object through StatusAggBatch's arrays, kad_sagg_check and the numpy restatement → (batch, outcome)."""
    b = SA.StatusAggBatch(kind)
    b.add(source, fed, objs)
    a = b.arrays()
    assert runtime.sagg_check(**a) == 0
    r = SA.sagg_numpy(**a) if b.device else None
    if b.device:
        want = R.run(**a)
        for k in want:
            assert np.array_equal(np.asarray(r[k]), np.asarray(want[k])), k
    return b, b.apply(r, now)[0]


def strip_times(status):
    for c in status.get("conditions", []):
        c["lastProbeTime"] = c["lastTransitionTime"] = None
    return status


# ------------------------------------------------------------------ the reference's table
@pytest.mark.parametrize("case", GOLDEN["cases"], ids=[c["name"] for c in GOLDEN["cases"]])
def test_golden(case):
    assert len(GOLDEN["cases"]) == 4
    objs = {c: copy.deepcopy(GOLDEN["jobs"][j]) for c, j in case["clusterObjs"].items()}
    src = copy.deepcopy(GOLDEN["jobs"][case["source"]])
    assert SA.aggregate_job(src, {}, objs, False, NOW) == case["expectedNeedUpdate"]
    assert strip_times(src["status"]) == case["expectedStatus"]
    new, need = R.job(copy.deepcopy(GOLDEN["jobs"][case["source"]]), objs, NOW)
    assert need == case["expectedNeedUpdate"] and strip_times(new) == case["expectedStatus"]
    src = copy.deepcopy(GOLDEN["jobs"][case["source"]])
    b, (need, err) = through_batch(SA.JOB, src, {}, objs)
    assert b.device == [0] and err is None and need == case["expectedNeedUpdate"]
    assert strip_times(src["status"]) == case["expectedStatus"]


# ------------------------------------------------------------------ Deployment
def dep(status, generation=1, annotations=None):
    return {"kind": "Deployment", "metadata": {"name": "d", "generation": generation, "annotations": annotations or {}},
            "status": status}


def member(replicas=3, ready=2, observed=4, **extra):
    return dict({"replicas": replicas, "updatedReplicas": replicas, "readyReplicas": ready, "availableReplicas": ready,
                 "unavailableReplicas": replicas - ready if type(replicas) is int and type(ready) is int else 0,
                 "observedGeneration": observed}, **extra)


def fed_of(*clusters, gen=4):
    return {"status": {"clusters": [{"name": n, "generation": gen, "status": "OK"} for n in clusters]}}


def run_dep(source, fed, objs, utd=True):
    """aggregate_deployment, the checker and the batch (with clusterObjsUpToDate forced) on copies → the source."""
    a, b = copy.deepcopy(source), copy.deepcopy(source)
    try:
        need = SA.aggregate_deployment(a, fed, objs, utd)
    except SA.StatusAggError:
        with pytest.raises(R.Err):
            R.deployment(b, fed, objs, utd)
        batch = SA.StatusAggBatch(SA.DEPLOYMENT)
        batch.add(b, fed, objs)
        assert 0 in batch.errors and batch.arrays()["obj_flags"][0] & SA.OBJ_ERROR
        assert batch.apply(SA.sagg_numpy(**batch.arrays()))[0][0] is False and b == source
        return None, None
    new, status_need = R.deployment(b, fed, objs, utd)
    assert R.go_equal(new, a["status"])
    batch = SA.StatusAggBatch(SA.DEPLOYMENT)
    batch.add(b, fed, objs)
    arr = batch.arrays()
    arr["obj_flags"] = (arr["obj_flags"] & np.uint8(0xFF ^ SA.OBJ_UPTODATE)) | np.uint8(SA.OBJ_UPTODATE if utd else 0)
    assert runtime.sagg_check(**arr) == 0
    r = SA.sagg_numpy(**arr)
    assert int(r["changed"][0]) == int(status_need)
    assert batch.apply(r)[0] == (need, None) and SA.deep_equal(a, b)
    return a, need


def test_deployment_sums_and_observed_generation():
    src = dep({"observedGeneration": 6.0}, generation=7)
    objs = {"c1": {"status": member()}, "c2": {"status": member(5, 5)}}
    got, need = run_dep(src, fed_of("c1", "c2"), objs)
    assert need and got["status"] == {"replicas": 8.0, "updatedReplicas": 8.0, "readyReplicas": 7.0, "availableReplicas": 7.0,
                                      "unavailableReplicas": 1.0, "observedGeneration": 7.0}
    # each way of clearing needUpdateObservedGeneration leaves the source's own observedGeneration
    for fed, o, utd in ((fed_of("c1", "c2"), objs, False),                                     # not up to date
                        (fed_of("c1", "c2"), dict(objs, c3={"status": None}), True),           # a nil status
                        (fed_of("c1"), objs, True),                                            # absent from status.clusters
                        (fed_of("c1", "c2", gen=5), objs, True),                               # generation differs
                        (None, objs, True)):
        got, _ = run_dep(src, fed, o, utd)
        assert got["status"]["observedGeneration"] == 6.0 and got["status"]["replicas"] == 8.0
    # a second pass over the written object changes nothing but is not asked to
    got, need = run_dep(run_dep(src, fed_of("c1", "c2"), objs)[0], fed_of("c1", "c2"), objs)
    assert not need


def test_deployment_errors_and_nil():
    src = dep({})
    for bad in ({}, {"status": "x"}, {"status": [1]},                       # not found, not a map
                {"status": member(replicas="3")}, {"status": member(replicas=True)}, {"status": member(replicas=1.5)},
                {"status": member(replicas=2 ** 31)}, {"status": member(replicas=-2 ** 31 - 1)},
                {"status": member(observed=2 ** 63)}, {"status": member(conditions="x")}, {"status": member(collisionCount="1")}):
        assert run_dep(src, fed_of("c1", "c2"), {"c1": {"status": member()}, "c2": bad}) == (None, None), bad
    # null fields, whole floats and unknown keys convert
    got, _ = run_dep(src, fed_of("c1"), {"c1": {"status": member(replicas=3.0, ready=None, extra="x", conditions=None)}})
    assert got["status"]["replicas"] == 3.0 and "readyReplicas" not in got["status"]
    # every member nil: an empty status, which differs from an absent one and equals an empty one
    got, need = run_dep(dep({}), fed_of("c1"), {"c1": {"status": None}})
    assert got["status"] == {} and got["metadata"]["annotations"][SA.RS_DIGESTS] == "[]"
    src = {"kind": "Deployment", "metadata": {"annotations": {SA.RS_DIGESTS: "[]"}}}
    got, need = run_dep(src, fed_of("c1"), {"c1": {"status": None}})
    assert need and got["status"] == {}
    assert run_dep(dict(src, status={}), fed_of("c1"), {"c1": {"status": None}})[1] is False
    assert run_dep(dict(src, status=None), fed_of("c1"), {}) == (None, None)  # the old status is not a map


def test_deployment_int32_wrap():
    objs = {"c1": {"status": member(2 ** 31 - 1, 0)}, "c2": {"status": member(1, 0)}, "c3": {"status": member(5, 0)}}
    got, _ = run_dep(dep({}), fed_of(), objs)
    assert got["status"]["replicas"] == float(-2 ** 31 + 5) == got["status"]["unavailableReplicas"]


def test_deployment_deep_equal_against_old_statuses():
    """GetUnstructuredStatus decodes the new status with encoding/json, so its numbers are float64: an old status
    equals it only with float64 values, no other key and no explicit zero."""
    objs = {"c1": {"status": member(3, 3, observed=0)}}
    same = {"replicas": 3.0, "updatedReplicas": 3.0, "readyReplicas": 3.0, "availableReplicas": 3.0}
    src = dep(same, annotations={SA.RS_DIGESTS: "[]"}, generation=0)
    assert run_dep(src, fed_of(), objs, utd=False)[1] is False
    for old in (dict(same, conditions=[]), dict(same, unavailableReplicas=0.0), dict(same, replicas=3), dict(same, replicas=4.0),
                {k: int(v) for k, v in same.items()}):
        got, need = run_dep(dep(old, annotations={SA.RS_DIGESTS: "[]"}, generation=0), fed_of(), objs, utd=False)
        assert need and got["status"] == same, old
    # an old status that does not convert to a DeploymentStatus fails the source's own conversion (deployment.go:53-56)
    for old in (dict(same, replicas=3.5), dict(same, replicas="3")):
        with pytest.raises(SA.StatusAggError):
            SA.aggregate_deployment(dep(old), fed_of(), objs, False)


def test_digests_eligibility_and_sort():
    def obj(gen, ann, status=None):
        return {"metadata": {"generation": gen, "annotations": ann}, "status": member() if status is None else status}
    full = {SA.RS_OBSERVED_GENERATION: "2", SA.RS_NAME: "rs-1", SA.RS_REPLICAS: "3", SA.RS_AVAILABLE: "0", SA.RS_READY: "2",
            SA.SOURCE_GENERATION: "9"}
    objs = {"zeta": obj(2, full), "alpha": obj(2, dict(full, **{SA.RS_NAME: 'q"<'})),
            "stale": obj(3, full),                                              # generation != observed-generation
            "no-name": obj(2, {k: v for k, v in full.items() if k != SA.RS_NAME}),
            "bad-int": obj(2, dict(full, **{SA.RS_REPLICAS: "3.0"})),
            "no-observed": obj(2, full, {"replicas": 1}),
            "nil": obj(2, full, False)}
    objs["nil"]["status"] = None
    text = SA.digests_annotation(objs)
    assert text == ('[{"clusterName":"alpha","replicasetName":"q\\"\\u003c","replicas":3,"readyReplicas":2,"observedGeneration":4,'
                    '"sourceGeneration":9},{"clusterName":"zeta","replicasetName":"rs-1","replicas":3,"readyReplicas":2,'
                    '"observedGeneration":4,"sourceGeneration":9}]')
    d, errs = SA.latest_replicaset_digest("c", objs["bad-int"])
    assert d["replicas"] == 0 and len(errs) == 1
    assert len(SA.latest_replicaset_digest("c", {"status": {}})[1]) == 6
    src = dep({})
    assert SA.aggregate_deployment(src, fed_of(), objs, False) and src["metadata"]["annotations"][SA.RS_DIGESTS] == text
    before = copy.deepcopy(src)
    assert SA.aggregate_deployment(src, fed_of(), objs, False) is False and src == before


# ------------------------------------------------------------------ IsResourcePropagated
def test_is_resource_propagated_exits():
    a, seg_cluster = synth.gen_status_aggregation(1, SA.DEPLOYMENT, 4, 6)
    a["obj_flags"][:] = SA.OBJ_UPTODATE
    (src, *_), (fed, *_), _ = synth.status_aggregation_objects(a, seg_cluster, [f"c{i}" for i in range(6)])
    src["metadata"].update(annotations={"a": "1", "b": "2"}, labels={"l": "x"})
    fed["metadata"]["annotations"].update({SA.OBSERVED_ANNOTATION_KEYS: "a|b", SA.OBSERVED_LABEL_KEYS: "l|", "a": "1"})
    fed["metadata"]["labels"] = {"l": "x"}
    fed["spec"]["template"] = {k: copy.deepcopy(v) for k, v in src.items() if k != "status"}
    assert SA.is_resource_propagated(src, fed) is True

    def with_(f):
        s, d = copy.deepcopy(src), copy.deepcopy(fed)
        f(s, d)
        return s, d

    with pytest.raises(SA.StatusAggError):
        SA.is_resource_propagated(None, fed)
    assert SA.is_resource_propagated(src, None) is False
    false_cases = [
        lambda s, d: d["spec"].pop("template"),
        lambda s, d: d["metadata"].pop("annotations"),
        lambda s, d: s["metadata"]["annotations"].update(c="3"),                     # a key nobody observed
        lambda s, d: d["metadata"]["annotations"].update(a="other"),                 # a federated key's value differs
        lambda s, d: d["metadata"]["annotations"].update({SA.OBSERVED_ANNOTATION_KEYS: "a,b"}),  # no separator
        lambda s, d: s["metadata"]["labels"].update(l="y"),
        lambda s, d: s["spec"].update(replicas=4),                                   # the template is behind
        lambda s, d: d["spec"]["template"]["spec"].update(replicas=3.0),             # DeepEqual is typed
        lambda s, d: d["status"].pop("syncedGeneration"),
        lambda s, d: d["status"].update(syncedGeneration=3),
        lambda s, d: d["status"]["clusters"].append({"name": "x", "status": "ClusterNotReady"}),
    ]
    for f in false_cases:
        assert SA.is_resource_propagated(*with_(f)) is False
    for f in (lambda s, d: d["spec"].update(template=[1]),
              lambda s, d: d["metadata"]["annotations"].update({SA.TEMPLATE_MERGE_PATCH: ""}),
              lambda s, d: d["status"].update(syncedGeneration="4")):
        with pytest.raises(SA.StatusAggError):
            SA.is_resource_propagated(*with_(f))
    # the merge patch prunes what the federate controller left out of the template
    s, d = with_(lambda s, d: (s["spec"].update(paused=True),
                               d["metadata"]["annotations"].update({SA.TEMPLATE_MERGE_PATCH: '{"status":null,"spec":{"paused":null}}'})))
    assert SA.is_resource_propagated(s, d) is True
    # the batch carries the result as UPTODATE
    b = SA.StatusAggBatch(SA.DEPLOYMENT)
    b.add(src, fed, {})
    b.add(*with_(false_cases[6]), {})
    assert b.arrays()["obj_flags"].tolist() == [SA.OBJ_UPTODATE, 0]


# ------------------------------------------------------------------ Job
def job(start=None, done=None, failed=False, status="True", **counts):
    st = dict(counts)
    if start is not None:
        st["startTime"] = start
    if done is not None:
        st["completionTime"] = done
    if failed:
        st["conditions"] = [{"type": "Complete", "status": "False"}, {"type": "Failed", "status": status}]
    return {"kind": "Job", "status": st}


T0, T1, T2 = "2024-01-01T00:00:00Z", "2024-01-01T00:00:10Z", "2024-01-01T00:01:00Z"


def run_job(source, objs):
    a, b = copy.deepcopy(source), copy.deepcopy(source)
    need = SA.aggregate_job(a, {}, objs, False, NOW)
    new, want_need = R.job(copy.deepcopy(source), objs, NOW)
    assert need == want_need and R.go_equal(new, a["status"] if need else new)
    batch, (bneed, err) = through_batch(SA.JOB, b, {}, objs)
    assert err is None and bneed == need and SA.deep_equal(a, b) and batch.device == [0]
    return a["status"], need


def test_job_classes_and_condition():
    src = {"kind": "Job", "metadata": {}, "status": {}}
    st, need = run_job(src, {"b": job(T1, T2, succeeded=2), "a": job(T0, T1, succeeded=1, failed=1)})
    assert need and st["conditions"][0]["message"] == "Job completed in clusters [a,b]" and st["completionTime"] == T2
    assert st["startTime"] == T0 and st["conditions"][0]["lastProbeTime"] == SA.format_time(NOW) and st["succeeded"] == 3
    st, _ = run_job(src, {"b": job(T1, failed=True, failed_=0), "a": job(T0, T1)})
    assert (st["conditions"][0]["reason"], st["conditions"][0]["type"]) == ("Mixed", "Failed") and "completionTime" not in st
    st, _ = run_job(src, {"b": job(T1, failed=True), "a": job(failed=True)})
    assert st["conditions"][0]["message"] == "Job failed in clusters [a,b]" and st["startTime"] == T1
    # not all finished: a running member, a Failed condition that is not True, a nil member counting in len(clusterObjs)
    for other in (job(T0, active=1), job(T0, failed=True, status="False"), {"status": None}):
        st, _ = run_job(src, {"a": job(T1, T2), "b": other})
        assert "conditions" not in st and "completionTime" not in st
    # a completed member with a Failed condition is completed
    st, _ = run_job(src, {"a": job(T0, T1, failed=True)})
    assert st["conditions"][0]["reason"] == "Completed"
    # nil start times never replace a set one, in either order; none set: no startTime
    assert run_job(src, {"a": job(), "b": job(T1), "c": job()})[0]["startTime"] == T1
    assert "startTime" not in run_job(src, {"a": job(), "b": {"status": None}})[0]
    # no members at all: an empty status, equal to the old one
    assert run_job(src, {}) == ({}, False)


def test_job_wrap_errors_and_old_statuses():
    src = {"kind": "Job", "metadata": {}, "status": {}}
    st, _ = run_job(src, {"a": job(active=2 ** 31 - 1), "b": job(active=1), "c": job(active=2 ** 32 + 7)})
    assert st["active"] == -2 ** 31 + 7  # int32 sums wrap; the converter sets an int64 without a range check
    for bad in ({}, {"status": 3}, job(active="1"), job(active=1.5), job(active=True), job(start=5), job(start="yesterday"),
                {"status": {"conditions": {}}}):
        b = SA.StatusAggBatch(SA.JOB)
        b.add(copy.deepcopy(src), {}, {"a": job(T0), "b": bad})
        assert 0 in b.errors, bad
        with pytest.raises(SA.StatusAggError):
            SA.aggregate_job(copy.deepcopy(src), {}, {"a": job(T0), "b": bad}, False, NOW)
        assert b.apply(SA.sagg_numpy(**b.arrays()), NOW)[0][0] is False
    objs = {"a": job(T0, active=1)}
    same = {"startTime": T0, "active": 1}
    assert run_job(dict(src, status=same), objs)[1] is False
    for old in (dict(same, ready=0), dict(same, failed=0), dict(same, active=1.0), dict(same, startTime="2024-01-01T01:00:00+01:00"),
                dict(same, conditions=[]), dict(same, completionTime=T1)):
        st, need = run_job(dict(src, status=old), objs)
        assert need and st == same, old
    # an appended condition is compared on the host: equal only with the same timestamps
    done = {"a": job(T0, T1)}
    st, _ = run_job(src, done)
    assert run_job(dict(src, status=st), done)[1] is False
    b, (need, _) = through_batch(SA.JOB, dict(src, status=copy.deepcopy(st)), {}, done, now=NOW + 1)
    assert need


def test_job_zero_time_and_subsecond_are_answered_by_the_host():
    src = {"kind": "Job", "metadata": {}, "status": {}}
    zero = "0001-01-01T00:00:00Z"
    for objs, why in (({"a": job(zero), "b": job(T1)}, SA.HOST_ZERO_TIME), ({"a": job("2024-01-01T00:00:00.5Z"), "b": job(T0)}, SA.HOST_SUBSECOND)):
        s = copy.deepcopy(src)
        b, (need, err) = through_batch(SA.JOB, s, {}, objs)
        assert b.host == {0: why} and b.device == [] and need and err is None
        want = copy.deepcopy(src)
        SA.aggregate_job(want, {}, objs, False, NOW)
        assert s == want
    # the order dependence that keeps the zero time off the device: a zero start is replaced by whatever follows
    s1, s2 = copy.deepcopy(src), copy.deepcopy(src)
    SA.aggregate_job(s1, {}, {"a": job(zero), "b": job(T1)}, False, NOW)
    SA.aggregate_job(s2, {}, {"b": job(T1), "a": job(zero)}, False, NOW)
    assert s1["status"]["startTime"] == T1 and s2["status"].get("startTime") is None
    # a zero completion time is not a completion
    s = copy.deepcopy(src)
    b, _ = through_batch(SA.JOB, s, {}, {"a": job(T0, zero)})
    assert b.device == [0] and s["status"] == {"startTime": T0}


# ------------------------------------------------------------------ kad_sagg_check, the route
def mutations(kind):
    base = SC.batch(kind, [2, 0, 3], seed=1)

    def mut(f):
        a = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in base.items()}
        f(a)
        return a

    out = [("kind", mut(lambda a: a.update(kind=2))),
           ("offsets start", mut(lambda a: a["obj_seg_off"].__setitem__(0, 1))),
           ("offsets order", mut(lambda a: a["obj_seg_off"].__setitem__(1, 4))),
           ("offsets end", mut(lambda a: a["obj_seg_off"].__setitem__(3, 4))),
           ("object flag", mut(lambda a: a["obj_flags"].__setitem__(0, 8))),
           ("segment flag", mut(lambda a: a["seg_flags"].__setitem__(0, 32))),
           ("other kind's flag", mut(lambda a: a["seg_flags"].__setitem__(0, R.START if kind == R.DEPLOYMENT else R.SYNCED)))]
    if kind == R.JOB:
        out += [("nil with start", mut(lambda a: a["seg_flags"].__setitem__(0, R.NIL | R.START))),
                ("done with failed", mut(lambda a: a["seg_flags"].__setitem__(0, R.DONE | R.FAILED))),
                ("start past the domain", mut(lambda a: (a["seg_flags"].__setitem__(0, R.START), a["seg_start"].__setitem__(0, SC.TMAX + 1)))),
                ("done before the domain", mut(lambda a: (a["seg_flags"].__setitem__(0, R.DONE), a["seg_done"].__setitem__(0, -SC.TMAX - 1)))),
                ("zero time", mut(lambda a: (a["seg_flags"].__setitem__(0, R.START), a["seg_start"].__setitem__(0, SA.TIME_ZERO))))]
    return base, out


@pytest.mark.parametrize("kind", [R.DEPLOYMENT, R.JOB])
def test_check_rules(kind):
    base, muts = mutations(kind)
    assert runtime.sagg_check(**base) == 0
    for name, a in muts:
        assert runtime.sagg_check(**a) == runtime.KAD_EINVAL, name
    if kind == R.JOB:  # a time behind a clear flag is not read
        a = dict(base, seg_flags=np.zeros_like(base["seg_flags"]), seg_start=np.full(5, 2 ** 62), seg_done=np.full(5, SA.TIME_ZERO))
        assert runtime.sagg_check(**a) == 0
    assert runtime.sagg_check(**SC.batch(kind, [])) == 0
    for k in ("obj_flags", "old_vals", "seg_vals"):  # a missing array
        b, v, keep, _ = runtime.sagg_args(**base)
        setattr(b, k, None)
        assert runtime.load_library().kad_sagg_check(runtime.ctypes.byref(b), runtime.ctypes.byref(v)) == runtime.KAD_EINVAL
    b, v, keep, _ = runtime.sagg_args(**base)
    v.changed = None
    assert runtime.load_library().kad_sagg_check(runtime.ctypes.byref(b), runtime.ctypes.byref(v)) == runtime.KAD_EINVAL


def test_route_boundaries():
    ev = runtime.sagg_route_eval
    lm = ev(1, 0, 1)["long_min"]
    assert lm >= 64 and ev(0, 0, 0)["grid"] == 0 and ev(5, 5, 0)["grid"] == 0 and ev(5, 5, 0)["long_grid"] == 5
    # width: mean segments per short object / 8, rounded up to a power of two in [1, 64]
    for mean, width in ((0, 1), (1, 1), (8, 1), (9, 2), (16, 2), (17, 4), (32, 4), (33, 8), (64, 8), (65, 16), (128, 16), (129, 32),
                        (256, 32), (257, 64), (512, 64), (100000, 64)):
        assert ev(1000, 0, 1000 * mean)["width"] == width, mean
    assert ev(1000, 0, 8001)["width"] == 2  # the mean rounds up
    assert ev(1001, 1, 8000)["width"] == 1  # long objects are left out of the mean
    r = ev(1000, 3, 4000, 256)
    assert r == {"width": 1, "long_min": lm, "threads": 256, "grid": 4, "long_grid": 3, "stride": 1024}
    r = ev(10 ** 6, 0, 3 * 10 ** 6, 256)
    assert r["grid"] == 2048 and r["stride"] == 2048 * 256  # capped at 8 blocks a CU
    assert ev(10 ** 6, 0, 3 * 10 ** 6, 4)["grid"] == 32
    out = (runtime.ctypes.c_int32 * 6)()
    L = runtime.load_library()
    for args in ((-1, 0, 0, 256), (1, 2, 0, 256), (1, 0, -1, 256), (1, 0, 0, 0)):
        assert L.kad_sagg_route_eval(*args, out) == runtime.KAD_EINVAL
    assert L.kad_sagg_route_eval(1, 0, 0, 256, None) == runtime.KAD_EINVAL


def test_header_and_exports_in_step():
    declared = [n for n in runtime.declared_functions() if "sagg" in n or n == "kad_status_aggregate"]
    assert sorted(declared) == ["kad_sagg_check", "kad_sagg_debug_route", "kad_sagg_last_route", "kad_sagg_route_eval",
                                "kad_sagg_timing", "kad_status_aggregate"]
    L = runtime.load_library()
    assert all(hasattr(L, n) for n in declared)


def test_synthetic_objects_round_trip_the_arrays():
    """synth's objects pack back into synth's arrays, and the batch path equals the per-object path."""
    names = [f"m{i:02d}" for i in range(12)]
    for kind in (SA.DEPLOYMENT, SA.JOB):
        a, seg_cluster = synth.gen_status_aggregation(5, kind, 120, len(names), duplicate_share=0.05, changed=0.3)
        srcs, feds, members = synth.status_aggregation_objects(a, seg_cluster, names)
        b = SA.StatusAggBatch(kind)
        for x in zip(srcs, feds, members):
            b.add(*x)
        a2 = b.arrays()
        assert not b.errors and not b.host
        for k, v in a.items():
            assert np.array_equal(np.asarray(v), np.asarray(a2[k])), k
        host = copy.deepcopy(srcs)
        outs = b.apply(SA.sagg_numpy(**a2), NOW)
        for i, (h, f, m) in enumerate(zip(host, feds, members)):
            utd = SA.is_resource_propagated(h, f)
            need = SA.aggregate_deployment(h, f, m, utd) if kind == SA.DEPLOYMENT else SA.aggregate_job(h, f, m, utd, NOW)
            assert outs[i] == (need, None) and SA.deep_equal(h, srcs[i]), i
