"""Rollout planning on the host: the reference's own table (tests/golden/rolloutplan.json) through the independent
checker (rollout_ref.py) and through rollout.py's prefix-sum restatement, the fencepost parser, every error path of
target construction, the action codes, the prefix-sum form against the serial walk (exhaustively on a small domain and
on seeded random objects), kad_rollout_check's rules and the ABI. No GPU."""
import copy
import itertools

import numpy as np
import pytest

import rollout_cases as RC
import rollout_ref as R
from kubeadmiral_amd import objects as O
from kubeadmiral_amd import rollout as RO
from kubeadmiral_amd import runtime, synth

CASES = RC.golden()
FTC = O.FederatedTypeConfig("apps", "v1", "Deployment", "deployments", "Namespaced", "spec.replicas", "status.replicas",
                            "status.readyReplicas", "status.availableReplicas", True)


def equal(got, want):
    assert set(got) == set(want)
    for k in want:
        assert np.asarray(got[k]).astype(np.int64).tolist() == list(want[k]), k


def test_golden_table_is_whole():
    assert len({c["func"] for c in CASES}) == 8 and len(CASES) >= 45
    assert all(set(t) == {"name", "updated", *R.FIELDS} for c in CASES for t in c["targets"])


@pytest.mark.parametrize("k", range(len(CASES)))
def test_golden_case(k):
    c = CASES[k]
    assert R.plan(c["replicas"], c["max_surge"], c["max_unavailable"], c["targets"]) == c["plans"]
    arr = RC.pack([RC.from_golden(c)])
    got = RO.plan_numpy(**arr)
    names = sorted((t["name"] for t in c["targets"]), key=lambda s: s.encode())
    assert RO.plans_of(got, 0, len(names), names) == c["plans"]
    equal(got, R.run(**arr))


# ------------------------------------------------------------------ the fencepost parser
def dep(surge=None, unavailable=None, prefix=()):
    ru = {k: v for k, v in (("maxSurge", surge), ("maxUnavailable", unavailable)) if v is not None}
    body = {"spec": {"strategy": {"rollingUpdate": ru}}}
    for f in reversed(prefix):
        body = {f: body}
    return body


@pytest.mark.parametrize("surge, unavailable, replicas, want", [
    (3, 2, 10, (3, 2)), ("25%", "25%", 10, (3, 2)), ("0%", "0%", 10, (0, 1)), (None, None, 10, (0, 1)),
    (-4, 2, 10, (0, 2)), (-1, 0, 10, (0, 0)), ("-10%", "50%", 10, (0, 5)), ("10%", "5%", 45, (5, 2)),
    (2.5, "100%", 7, (0, 7)), (0, 0, 0, (0, 1)), ("+50%", None, 3, (2, 0))])
def test_retrieve_fencepost(surge, unavailable, replicas, want):
    assert RO.retrieve_fencepost(dep(surge, unavailable), RO.MAX_SURGE_FIELDS, RO.MAX_UNAVAILABLE_FIELDS, replicas) == want


@pytest.mark.parametrize("bad", ["25", "abc%", "%", "1.5%", "२५%"])
def test_fencepost_string_must_be_a_percentage(bad):
    with pytest.raises(RO.RolloutError):
        RO.retrieve_fencepost(dep(bad, 1), RO.MAX_SURGE_FIELDS, RO.MAX_UNAVAILABLE_FIELDS, 10)


def test_fencepost_under_a_non_map_is_absent():
    assert RO.retrieve_fencepost({"spec": {"strategy": "Recreate"}}, RO.MAX_SURGE_FIELDS, RO.MAX_UNAVAILABLE_FIELDS, 10) == (0, 1)


# ------------------------------------------------------------------ target construction
def member(replicas=10, revision="r2", rs=("rs-b", "7", "6"), last=None, available=9, **spec):
    ann = {RO.CURRENT_REVISION_ANNOTATION: revision, RO.LATEST_RS_NAME: rs[0], RO.LATEST_RS_REPLICAS: rs[1],
           RO.LATEST_RS_AVAILABLE: rs[2]}
    if last is not None:
        ann[RO.LAST_REPLICASET_NAME] = last
    return {"metadata": {"annotations": ann}, "spec": dict({"replicas": replicas, "strategy": {"rollingUpdate": {"maxSurge": "20%"}}}, **spec),
            "status": {"replicas": 12, "availableReplicas": available}}


def test_target_info():
    t = RO.target_info("c1", member(), 8, "r2", FTC)
    # ActualReplicas is the spec's replicas (read from the ReplicasSpec path twice), not status.replicas
    assert t == dict(name="c1", updated=True, exists=True, replicas=10, actual=10, available=9, updated_replicas=7,
                     updated_available=6, current_new=7, current_new_available=6, max_surge=2, max_unavailable=0, desired=8)
    t = RO.target_info("c1", member(revision="r1"), 8, "r2", FTC)
    assert (t["updated"], t["updated_replicas"], t["updated_available"], t["current_new"]) == (False, 0, 0, 7)
    t = RO.target_info("c1", member(last="rs-b"), 8, "r2", FTC)  # the annotations lag behind the template
    assert (t["current_new"], t["current_new_available"], t["updated_replicas"]) == (0, 0, 0)
    t = RO.target_info("c1", None, 8, "r2", FTC)
    assert not t["exists"] and all(t[f] == 0 for f in R.FIELDS[:-1]) and t["desired"] == 8
    m = member()
    del m["status"]["availableReplicas"]
    assert RO.target_info("c1", m, 8, "r2", FTC)["available"] == 0


def _without(key):
    m = member()
    del m["metadata"]["annotations"][key]
    return m


@pytest.mark.parametrize("obj, message", [
    (member(replicas=None), "failed to retrieve replicas"), (member(replicas="3"), "failed to retrieve replicas"),
    ({"metadata": {}, "spec": 5}, "failed to retrieve replicas"),
    (member(strategy={"rollingUpdate": {"maxSurge": "x"}}), "failed to retrieve fencepost"),
    (_without(RO.CURRENT_REVISION_ANNOTATION), "failed to retrieve annotation"),
    (_without(RO.LATEST_RS_REPLICAS), "missing annotation latestreplicaset.kubeadmiral.io/replicas"),
    (_without(RO.LATEST_RS_AVAILABLE), "missing annotation latestreplicaset.kubeadmiral.io/available-replicas"),
    (_without(RO.LATEST_RS_NAME), "missing annotation latestreplicaset.kubeadmiral.io/name"),
    (member(rs=("rs", "", "1")), "missing annotation"), (member(rs=("rs", "1.5", "1")), "invalid syntax"),
    (member(rs=("rs", "1", str(2 ** 31))), "out of range"),
    (member(available="9"), "failed to retrieve actual available replicas")])
def test_target_info_errors(obj, message):
    if obj["spec"] != 5 and obj["spec"].get("replicas") is None:
        del obj["spec"]["replicas"]
    with pytest.raises(RO.RolloutError, match=message):
        RO.target_info("c1", obj, 1, "r2", FTC)


def fed_object(overrides=None, template_replicas=4, revision="r2", **spec):
    meta = {"annotations": {RO.CURRENT_REVISION_ANNOTATION: revision}} if revision else {}
    tmpl = {"spec": {"strategy": {"rollingUpdate": {"maxSurge": "25%", "maxUnavailable": 0}}}}
    if template_replicas is not None:
        tmpl["spec"]["replicas"] = template_replicas
    return {"metadata": meta, "spec": dict({"template": tmpl, "overrides": overrides or []}, **spec)}


def test_driver_replicas_and_planner():
    ov = [{"controller": "b", "clusters": [{"clusterName": "c1", "patches": [{"path": "/spec/replicas", "value": 7.0}]}]},
          {"controller": "a", "clusters": [{"clusterName": "c1", "patches": [{"path": "/spec/replicas", "value": 3.9}]},
                                           {"clusterName": "c2", "patches": [{"path": "/spec/replicas", "value": None},
                                                                             {"path": "/x", "value": 1}]}]}]
    fed = fed_object(ov)
    assert RO.replicas_override_for_cluster(fed, FTC, "c1") == 7
    assert RO.replicas_override_for_cluster(fed, FTC, "c1", RO.overrides_map(fed, ["a", "b"])) == 3  # float64 → int32
    assert RO.replicas_override_for_cluster(fed, FTC, "c2") == 4 and RO.total_replicas(fed, FTC, {"c1", "c2", "c3"}) == 15
    assert RO.new_planner(fed, 15) == (4, 0, "r2")
    bad = fed_object([{"controller": "a", "clusters": [{"clusterName": "c1", "patches": [{"path": "/spec/replicas", "value": "7"}]}]}])
    with pytest.raises(RO.RolloutError, match="failed to retrieve replicas override for c1"):
        RO.total_replicas(bad, FTC, {"c1"})
    with pytest.raises(RO.RolloutError, match="failed to retrieve replicas override for c9"):
        RO.replicas_override_for_cluster(fed_object(template_replicas=None), FTC, "c9")
    with pytest.raises(RO.RolloutError, match="from federated resource"):
        RO.new_planner(fed_object(revision=None), 3)
    assert RO.check_retain_replicas(fed_object(retainReplicas=True)) and not RO.check_retain_replicas(fed)
    with pytest.raises(RO.RolloutError):
        RO.check_retain_replicas(fed_object(retainReplicas="yes"))


def test_batch_packs_the_driver():
    b = RO.RolloutBatch(FTC)
    objs = {"c2": member(), "c1": member(revision="r1"), "c0": member(), "gone": dict(member(), metadata={"deletionTimestamp": "t"}),
            "new": None, "absent": None}
    b.add(fed_object(), objs, {"c1", "c2", "new"})
    b.add(fed_object(revision=None), {"c1": member(), "c3": None}, {"c1", "c3"})
    b.add(fed_object(), {"c1": member()}, {"c1"})
    b.ftc = O.FederatedTypeConfig("apps", "v1", "StatefulSet", replicas_spec="spec.replicas")
    b.add(fed_object(), {"c1": member()}, {"c1"})
    a = b.arrays()
    assert a["obj_tgt_off"].tolist() == [0, 4, 6, 7, 8] and a["obj_flags"].tolist() == [0, 1, 0, 1]
    assert [t["name"] for t in b.targets[:4]] == ["c0", "c1", "c2", "new"]  # "gone" waits for removal, "absent" is not selected
    assert a["tgt_flags"][:6].tolist() == [R.UPDATED | R.EXISTS | R.TO_DELETE, R.EXISTS, R.UPDATED | R.EXISTS, 0, R.EXISTS, 0]
    assert a["tgt_vals"][9, :4].tolist() == [0, 4, 4, 4] and a["obj_replicas"].tolist() == [12, 0, 4, 0]
    assert "Unsupported target type" in b.errors[3] and "current-revision" in b.errors[1]
    rc, nowrap = runtime.rollout_check(**a)
    assert rc == 0 and nowrap.all()
    out = b.apply(R.run(**a))
    assert [o.status for o in out] == [R.OK, R.ERROR, R.OK, R.ERROR]
    assert out[1].actions == {"c1": R.KEEP_TEMPLATE_PATCH, "c3": R.NONE} and out[1].plans == {} and out[1].error
    assert out[0].overrides["c1"] == RO.to_overrides(out[0].plans.get("c1"))


def test_to_overrides():
    assert RO.to_overrides(None) == [] and RO.to_overrides(R._new()) == []
    p = {"replicas": 3, "max_surge": None, "max_unavailable": 0, "only_patch_replicas": True}
    assert RO.to_overrides(p) == [{"path": "/spec/replicas", "value": 3},
                                  {"path": "/spec/strategy/rollingUpdate/maxUnavailable", "value": 0}]


def test_action_codes():
    """managed.go:219-249, branch by branch, through the restatement's columns and the checker."""
    plan = lambda r=None, only=False: {"replicas": r, "max_surge": None, "max_unavailable": None, "only_patch_replicas": only}  # noqa: E731
    E, D = R.EXISTS, R.TO_DELETE
    table = [(E, None, R.KEEP_TEMPLATE_PATCH), (0, None, R.NONE), (E | D, plan(), R.DELETE), (E | D, plan(0), R.DELETE),
             (E | D, plan(2, True), R.PATCH_REPLICAS), (E | D, plan(2), R.UPDATE), (0, plan(3), R.CREATE),
             (E, plan(3, True), R.PATCH_REPLICAS), (E, plan(None, True), R.UPDATE), (E, plan(3), R.UPDATE)]
    for flags, p, want in table:
        assert R.action(flags, p) == want, (flags, p)
    _, marks, want = _shapes()
    assert set(want["action"]) == set(range(6))  # the shapes reach every action


_cache = []


def _shapes():
    if not _cache:
        arr, marks = RC.shapes_case(runtime.rollout_route_eval(1, 0, 1)["long_min"])
        _cache.append((arr, marks, R.run(**arr)))
    return _cache[0]


# ------------------------------------------------------------------ the prefix-sum form == the serial walk
def test_prefix_form_equals_serial_walk_on_the_shapes():
    arr, marks, want = _shapes()
    rc, nowrap = runtime.rollout_check(**arr)
    assert rc == 0
    lib = RO.nowrap(**arr)
    assert (lib == (nowrap != 0)).all() and 9 <= int((~lib).sum()) < 20
    keep = np.flatnonzero(lib)
    objs_off = arr["obj_tgt_off"]
    sel = np.concatenate([np.arange(objs_off[o], objs_off[o + 1]) for o in keep]) if len(keep) else np.zeros(0, np.int64)
    sub = {"obj_tgt_off": np.concatenate(([0], np.cumsum(np.diff(objs_off)[keep]))).astype(np.int32),
           "tgt_vals": arr["tgt_vals"][:, sel], "tgt_flags": arr["tgt_flags"][sel],
           **{k: arr[k][keep] for k in ("obj_max_surge", "obj_max_unavailable", "obj_replicas", "obj_flags")}}
    got = RO.plan_numpy(**sub)
    for k in ("replicas", "max_surge", "max_unavailable", "plan_flags", "action"):
        assert got[k].tolist() == [want[k][i] for i in sel], k
    assert got["status"].tolist() == [want["status"][o] for o in keep]
    with pytest.raises(ValueError):
        RO.plan_numpy(**arr)


def test_prefix_form_equals_serial_walk_on_random_objects():
    for seed in range(3):
        arr = RC.batch(np.random.default_rng(seed).integers(0, 12, 400).tolist(), seed=seed)
        equal(RO.plan_numpy(**arr), R.run(**arr))
    a = synth.gen_rollout(3, 800, 1, 33)
    got = RO.plan_numpy(**a)
    equal(got, R.run(**a))
    planned = np.add.reduceat((got["plan_flags"] & R.PLANNED).astype(np.int64), a["obj_tgt_off"][:-1])
    assert ((got["status"] == R.OK) & (planned > 0)).mean() >= 0.8


def _small_targets():
    """Every target over a small value domain: replicas, desired, the new replica set and the deviations 0..2, the
    member's fenceposts 0..1."""
    out = []
    for r, d, upd, new, dev, ms, mu in itertools.product((0, 1, 2), (0, 1, 2), (False, True), (0, 1, 2), (-1, 0, 1), (0, 1), (0, 1)):
        if new > r:
            continue
        out.append(RC.tgt(r, d, upd, new, max(0, new - (dev == 1)), max(0, r + dev), max(0, r - (dev != 0)), ms, mu))
    return out


def test_prefix_form_equals_serial_walk_exhaustively():
    """Every object of one target over the small domain and six template settings, every pair of targets over a thinned
    domain, every triple over a further thinned one: the prefix-sum form, evaluated in one batch, equals the serial
    walk object by object."""
    ts = _small_targets()
    settings = [(rep, ms, mu) for rep in (1, 3) for ms, mu in ((0, 1), (1, 0), (1, 1))]
    objs = [RC.obj(rep, ms, mu, [t]) for t in ts for rep, ms, mu in settings]
    t2, t3 = ts[::7], ts[::41]
    objs += [RC.obj(rep, ms, mu, [a, b]) for a in t2 for b in t2 for rep, ms, mu in settings[1::2]]
    objs += [RC.obj(rep, ms, mu, [a, b, c]) for a in t3 for b in t3 for c in t3 for rep, ms, mu in ((4, 1, 1), (2, 0, 1))]
    assert len(objs) > 15000
    arr = RC.pack(objs)
    assert RO.nowrap(**arr).all()
    equal(RO.plan_numpy(**arr), R.run(**arr))


def test_nowrap_rejects_sums_that_reach_2_31():
    small = RC.obj(10, 1, 1, [RC.tgt(5, 5), RC.tgt(5, 5)])
    edge = 2 ** 29
    cases = [(small, True), (RC.obj(edge - 1 - 60, 0, 0, [RC.tgt(10, 10)]), True), (RC.obj(edge - 60, 0, 0, [RC.tgt(10, 10)]), False),  # (a target sums to 60)
             (RC.obj(2 ** 31 - 1, 0, 0, []), False), (RC.obj(0, 0, 0, [RC.tgt(-2 ** 31, 0)]), False),
             (RC.obj(0, 0, 0, [RC.tgt(2 ** 30, 2 ** 30, actual=0, available=0)] * 2), False)]
    arr = RC.pack([o for o, _ in cases])
    rc, nowrap = runtime.rollout_check(**arr)
    assert rc == 0 and nowrap.tolist() == [int(w) for _, w in cases]
    assert RO.nowrap(**arr).tolist() == [w for _, w in cases]


# ------------------------------------------------------------------ kad_rollout_check, the route, the ABI
def test_check_rejects_malformed_batches():
    good = RC.batch([3, 0, 2], seed=1)
    assert runtime.rollout_check(**good)[0] == 0

    def bad(**change):
        a = copy.deepcopy(good)
        a.update(change)
        return runtime.rollout_check(**a)[0]

    off = good["obj_tgt_off"]
    assert bad(obj_tgt_off=off + 1) == runtime.KAD_EINVAL                        # not from 0
    assert bad(obj_tgt_off=np.array([0, 3, 2, 5], np.int32)) == runtime.KAD_EINVAL  # decreasing
    assert bad(obj_tgt_off=np.array([0, 3, 3, 4], np.int32)) == runtime.KAD_EINVAL  # does not end at n_targets
    assert bad(obj_flags=np.array([0, 2, 0], np.uint8)) == runtime.KAD_EINVAL
    f = good["tgt_flags"].copy()
    f[0] = 8
    assert bad(tgt_flags=f) == runtime.KAD_EINVAL
    f[0] = R.UPDATED  # UPDATED without EXISTS
    assert bad(tgt_flags=f) == runtime.KAD_EINVAL
    f[0] = 0  # no object, but a status
    v = good["tgt_vals"].copy()
    v[0, 0] = 3
    assert bad(tgt_flags=f, tgt_vals=v) == runtime.KAD_EINVAL
    f[0] = R.EXISTS | R.TO_DELETE
    v[9, 0] = 1  # to delete, but desired
    assert bad(tgt_flags=f, tgt_vals=v) == runtime.KAD_EINVAL
    v[9, 0] = 0
    assert bad(tgt_flags=f, tgt_vals=v) == 0
    L = runtime.load_library()
    b, view, _keep, _ = runtime.rollout_args(**good)
    assert L.kad_rollout_check(None, runtime.ctypes.byref(view), None) == runtime.KAD_EINVAL
    assert L.kad_rollout_check(runtime.ctypes.byref(b), None, None) == runtime.KAD_EINVAL
    view.status = None
    assert L.kad_rollout_check(runtime.ctypes.byref(b), runtime.ctypes.byref(view), None) == runtime.KAD_EINVAL
    b.n_objects = -1
    assert L.kad_rollout_check(runtime.ctypes.byref(b), None, None) == runtime.KAD_EINVAL
    for missing in ("obj_tgt_off", "obj_replicas", "tgt_vals", "tgt_flags"):
        b, view, _keep, _ = runtime.rollout_args(**good)
        setattr(b, missing, None)
        assert L.kad_rollout_check(runtime.ctypes.byref(b), runtime.ctypes.byref(view), None) == runtime.KAD_EINVAL, missing
    assert runtime.rollout_check(**RC.pack([]))[0] == 0


def test_route():
    ev = runtime.rollout_route_eval
    assert [ev(100, 0, 100 * m)["width"] for m in (0, 1, 2, 3, 8, 9, 33, 64, 500)] == [1, 1, 2, 4, 8, 16, 64, 64, 64]
    r = ev(1000, 10, 8000, 3, 256)
    assert (r["long_min"], r["threads"], r["long_grid"], r["serial"]) == (256, 256, 3, 3)
    assert r["width"] == 16 and r["stride"] == r["grid"] * (256 // r["width"])  # 8000 targets on 990 short objects
    assert ev(10 ** 7, 0, 8 * 10 ** 7)["grid"] == 256 * 8 and ev(5, 5, 0)["grid"] == 0
    for args in ((-1, 0, 0), (1, 2, 0), (1, 0, -1), (1, 0, 0, 2), (1, 0, 0, 0, 0)):
        with pytest.raises(ValueError):
            ev(*args)


def test_abi_exports():
    declared = [n for n in runtime.declared_functions() if "rollout" in n]
    assert sorted(declared) == ["kad_rollout_check", "kad_rollout_debug_route", "kad_rollout_last_route", "kad_rollout_plan",
                                "kad_rollout_route_eval", "kad_rollout_timing"]
    L = runtime.load_library()
    assert all(hasattr(L, n) for n in declared)
    ftc = O.FederatedTypeConfig("apps", "v1", "Deployment")
    assert (ftc.available_replicas_status, ftc.rollout_plan) == ("", False)
