"""Sync completion without a GPU: the field reads of ObjectNeedsUpdate, the version rules, SyncFinishBatch's packing
with the numpy restatements against the per-object checker (syncfin_ref.py) on the named and seeded cases and on the
cases of the reference's status_test.go, and the library's validation and launch decisions."""
import numpy as np
import pytest

import syncfin_cases as SC
import syncfin_ref as R
from kubeadmiral_amd import syncfin as SF


@pytest.fixture(scope="module")
def runtime():
    from kubeadmiral_amd import build, runtime
    build.build()
    return runtime


def split(arrays, keys):
    return [arrays[k] for k in keys], {k: v for k, v in arrays.items() if k not in keys}


FIN_HEAD = ("n_clusters", "n_reasons", "reason_check_clusters", "reason_ns_not_federated")


def test_constants():
    assert SF.STATUS_NAMES[1:] == SC.STATUSES and len(SF.STATUS_NAMES) == SF.ST_MAX + 1 == 24
    assert [SF.STATUS_NAMES[i] for i in (1, 2, 20, 21, 22, 23)] == \
        ["OK", "WaitingForRemoval", "CreationTimedOut", "UpdateTimedOut", "DeletionTimedOut", "LabelRemovalTimedOut"]
    assert SF._TRANSITION.tolist() == [SF.STATUS_CODE[SC.AFTER_WAIT.get(s, s)] for s in SF.STATUS_NAMES]


def test_object_version():
    assert SF.object_version({"metadata": {"generation": 3, "resourceVersion": "9"}}) == "gen:3"
    assert SF.object_version({"metadata": {"generation": 0, "resourceVersion": "9"}}) == "rv:9"
    assert SF.object_version({"metadata": {"resourceVersion": "9"}}) == "rv:9"
    assert SF.object_version({}) == "rv:"
    for m in ({"metadata": {"generation": -1}}, {"metadata": {"resourceVersion": "12"}}):
        assert SF.object_version(m) == R.object_version(m)


@pytest.mark.parametrize("version,want", [("gen:5", 5), ("gen:+5", 5), ("gen:05", 5), ("gen:", None),
                                          ("gen:9223372036854775808", None), ("gen:9223372036854775807", 2 ** 63 - 1),
                                          ("gen:-9223372036854775808", -2 ** 63), ("gen:-9223372036854775809", None),
                                          ("gen:1_0", None), ("gen: 5", None), ("gen:5\n", None), ("gen:٥", None),
                                          ("rv:x", 0), ("rv:", 0), ("x", None), ("", None)])
def test_generation_of_version(version, want):
    assert SF.generation_of_version(version) == want
    assert R.generation_map({"c": version}) == ({} if want is None else {"c": want})
    assert SF.version_flags(version)[0] == (0 if want is None else 1) | (2 if version.startswith("gen:") else 0)


def test_propagated_versions_store():
    pv = SF.PropagatedVersions("Deployment")
    assert SF.propagated_version_name("Deployment", "web") == "deployment-web" and pv.status("ns", "web") is None
    assert pv.get("ns", "web", "t", "o") == {}
    st = SC.stored([("a", "gen:1"), ("b", "rv:2"), ("a", "gen:9")], "t", "o")
    o = pv.set_status("ns", "web", st)
    assert o["metadata"] == {"name": "deployment-web", "namespace": "ns"} and pv.status("ns", "web") is st
    assert pv.get("ns", "web", "t", "o") == {"a": "gen:9", "b": "rv:2"} == R.version_get(st, "t", "o")
    assert pv.get("ns", "web", "t2", "o") == {} and pv.get("ns", "web", "t", "o2") == {}
    pv.delete("ns", "web")
    assert pv.status("ns", "web") is None


M = SC.member
NEEDS_UPDATE = [  # (desired, member, recorded version, needs update)
    (M(), M(2), "gen:2", False), (M(), M(2), "gen:1", True), (M(), M(2), "", True), (M(), M(0, "7"), "rv:7", False),
    (M(replicas=1), M(2, replicas=1), "gen:2", False), (M(replicas=1), M(2, replicas=2), "gen:2", True),
    (M(replicas=1), M(2), "gen:2", True), (M(), M(2, replicas=1), "gen:2", True),
    (M(replicas="1"), M(2, replicas="1"), "gen:2", True), (M(replicas=1), M(2, replicas=1.0), "gen:2", True),
    (M(surge="25%"), M(2, surge="25%"), "gen:2", False), (M(surge="25%"), M(2, surge="30%"), "gen:2", True),
    (M(surge="25%"), M(2), "gen:2", True), (M(), M(2, surge=""), "gen:2", True), (M(surge="25%"), M(2, surge=1), "gen:2", True),
    (M(surge=1), M(2, surge=1), "gen:2", False), (M(surge=1), M(2, surge=2), "gen:2", True), (M(surge=1), M(2), "gen:2", True),
    (M(surge=0), M(2), "gen:2", True), (M(surge=1), M(2, surge="1"), "gen:2", True), (M(surge=1.5), M(2, surge=1.5), "gen:2", True),
    (M(), M(2, surge=1), "gen:2", True),  # the string read of the desired object does not err: the int64 branch is skipped
    (M(unavailable="1"), M(2, unavailable="1"), "gen:2", False), (M(unavailable=1), M(2, unavailable=1), "gen:2", False),
    (M(unavailable=1), M(2, unavailable=3), "gen:2", True), (M(unavailable="1"), M(2), "gen:2", True),
    (M(labels={"a": "b"}), M(2, labels={"a": "b"}), "gen:2", False), (M(labels={"a": "b"}), M(2, labels={"a": "c"}), "gen:2", True),
    (M(labels={}), M(2), "gen:2", False), (M(labels={"a": "b"}), M(0, "7", labels={"a": "c"}), "rv:7", False),
    (M(name="y"), M(2), "gen:2", True),
]


@pytest.mark.parametrize("k", range(len(NEEDS_UPDATE)))
def test_object_needs_update_branches(k):
    desired, member, recorded, want = NEEDS_UPDATE[k]
    assert R.needs_update(desired, member, recorded, "spec.replicas") == want
    b = SC.pack_rows(["c1"], [(SC.stored([("c1", recorded)]) if recorded else None, "t1", "o1")], [(0, "c1", desired, member)])
    got = b.apply_needs_update(SF.needs_update_numpy(**b.needs_update_arrays()))
    assert got == [{"c1": (want, recorded)}]


def test_needs_update_quirks():
    # an intermediate that is no map errs; an empty replicas path reads the object itself and errs: always an update
    assert SF.needs_update_flags({"spec": 1}, {"spec": 1}, "spec.replicas") == SF.ROW_META_EQUIVALENT
    assert SF.needs_update_flags(M(), M(), "") & SF.ROW_REPLICAS_EQUAL == 0 and R.needs_update(M(), M(2), "gen:2", "")
    assert SF.needs_update_flags(M(), M(), "spec.replicas") == 15


@pytest.mark.parametrize("seed", range(4))
def test_needs_update_numpy_equals_the_reference(seed):
    cl, objects, rows = SC.update_rows(seed, 9, 40, 5)
    b = SC.pack_rows(cl[::-1], objects, rows)
    res = SF.needs_update_numpy(**b.needs_update_arrays())
    assert SC.compare_rows(b, res, objects, rows) is None
    assert 0 < res["needs_update"].sum() < len(rows) and (res["recorded"] != 0).any()


def golden_object(g, case):
    records = {n: (s, "") for n, s in case["statusMap"].items()}
    for n, gen in case["generationMap"].items():
        records[n] = (records.get(n, ("", ""))[0], "gen:%d" % gen if gen else "rv:1")
    return SC.obj(records, status=g["storedStatus"], generation=case["generation"], collision=case["collisionCount"],
                  resources_updated=case["resourcesUpdated"], reason=case["reason"])


def test_golden_cases():
    g = SC.golden()
    assert len(g["cases"]) == 5
    objs = [golden_object(g, c) for c in g["cases"]]
    assert [R.finish(o)["status_write"] for o in objs] == [c["expectedChanged"] for c in g["cases"]]
    b = SC.pack(["cluster1"], objs)
    res = SF.finish_numpy(**b.finish_arrays())
    assert [bool(x & SF.OUT_STATUS_WRITE) for x in res["obj_out"]] == [c["expectedChanged"] for c in g["cases"]]
    assert SC.compare(b, res, objs) is None


@pytest.mark.parametrize("name", sorted(SC.named()))
def test_finish_numpy_on_the_named_cases(name):
    cl, objs = SC.named()[name]
    b = SC.pack(cl, objs)
    assert SC.compare(b, SF.finish_numpy(**b.finish_arrays()), objs) is None


def test_named_cases_hit_their_corners():
    n = SC.named()
    f = lambda name, k=0: R.finish(n[name][1][k])  # noqa: E731
    assert f("generation_map_length")["clusters_changed"] and f("generation_unparsed")["clusters_changed"]
    assert not f("unchanged")["status_write"] and f("unchanged_resources_updated")["status_write"]
    assert not f("resources_updated_empty_map")["status_write"] and not f("all_label_removal")["status_write"]
    assert not f("oldv_equal")["version_write"] and f("oldv_equal_other_version")["version_write"]
    assert [f("oldv_nil_and_empty", k)["version_write"] for k in range(4)] == [True, False, True, True]
    assert all(f("oldv_irregular", k)["version_write"] for k in range(5)) and not f("olds_unordered")["clusters_changed"]
    assert not f("status_on_host_between", 1)["clusters_changed"]  # [a, a] against {a, b}
    writes = [R.finish(o)["status_write"] for o in n["condition_transitions"][1]]
    assert any(writes) and not all(writes)


@pytest.mark.parametrize("seed,C,n,size,irr", [(1, 1, 30, 1, 0), (2, 7, 120, 7, 0), (3, 64, 60, 40, 9), (4, 65, 60, 65, 8),
                                               (5, 300, 40, 200, 0)])
def test_finish_numpy_on_random_batches(seed, C, n, size, irr):
    cl, objs = SC.random_batch(seed, C, n, size, irr)
    hosted = sum(SC.is_on_host(o, set(cl)) for o in objs)
    assert hosted * 8 <= len(objs) and (hosted > 0) == (irr > 0 and C > 1)
    b = SC.pack(cl, objs)
    a = b.finish_arrays()
    assert int(((a["obj_flags"] & SF.OBJ_STATUS_ON_HOST) != 0).sum()) == hosted
    assert SC.compare(b, SF.finish_numpy(**a), objs) is None
    want = [R.finish(o) for o in objs]
    if 1 < size <= 7:
        for field in ("version_write", "status_write", "clusters_changed"):
            assert len({w[field] for w in want}) == 2, field


def test_generator_never_makes_irregular_lists_unasked():
    for seed in range(20):
        cl, objs = SC.random_batch(100 + seed, 20, 50, 12)
        assert not any(SC.is_on_host(o, set(cl)) for o in objs)
        assert not (SC.pack(cl, objs).finish_arrays()["obj_flags"] & (SF.OBJ_STATUS_ON_HOST | SF.OBJ_OLDV_IRREGULAR)).any()


def test_cluster_ids_follow_the_byte_order_of_the_names():
    b = SF.SyncFinishBatch(["b", "a", "B", "ab", "é", "a"])
    assert b.names == ["B", "a", "ab", "b", "é"]


def fin_arrays():
    cl, objs = SC.named()["oldv_interleaved"]
    both = objs + SC.named()["unchanged"][1] + SC.named()["condition_transitions"][1][:3]
    return {k: (np.array(v) if isinstance(v, np.ndarray) else v) for k, v in SC.pack(cl, both).finish_arrays().items()}


def fin_check(runtime, arrays):
    head, rest = split(arrays, FIN_HEAD)
    return runtime.sync_finish_check(*head, **rest)


def test_finish_validation(runtime):
    a = fin_arrays()
    assert fin_check(runtime, a) == 0
    assert len(a["ent_cluster"]) >= 3 and len(a["oldv_cluster"]) >= 5 and len(a["olds_cluster"]) >= 2
    V, O = len(a["ver_flags"]), len(a["obj_flags"])

    def patched(key, index, value):
        x = a[key].copy()
        x[index] = value
        return {key: x}

    bad = [
        patched("ent_cluster", 1, a["ent_cluster"][0]), patched("ent_cluster", 0, a["ent_cluster"][1] + 1),   # not strictly ascending
        patched("oldv_cluster", 1, a["oldv_cluster"][0]), patched("sel_cluster", 1, a["sel_cluster"][0]),
        patched("olds_cluster", 1, a["olds_cluster"][0]),
        patched("ent_cluster", 0, -1), patched("ent_cluster", len(a["ent_cluster"]) - 1, a["n_clusters"]),       # an id outside [0, C)
        patched("sel_cluster", 0, -1), patched("oldv_cluster", 4, a["n_clusters"]), patched("olds_cluster", 0, -5),
        patched("ent_version", 0, V), patched("ent_version", 0, -1), patched("oldv_version", 0, V), patched("oldv_version", 0, 0),
        patched("ent_status", 0, 24), patched("olds_status", 0, 0), patched("olds_status", 0, 24),              # an unknown status code
        patched("obj_flags", 0, 512), patched("obj_flags", 0, SF.OBJ_VERSIONS_CURRENT), patched("obj_flags", 0, SF.OBJ_COND_TRUE),
        patched("obj_flags", 0, int(a["obj_flags"][0]) | SF.OBJ_OLDV_NIL), patched("obj_flags", 1, int(a["obj_flags"][1]) | SF.OBJ_STATUS_ON_HOST),
        patched("ver_flags", 1, 4), patched("ver_flags", 0, 1),
        patched("reason_in", 0, a["n_reasons"]), patched("reason_in", 0, -1), patched("cond_reason", 0, -2),
        {"ver_off": a["ver_off"] - (np.arange(O + 1) > 0)},                              # a capacity below the bound
        {"st_off": np.minimum(a["st_off"], a["st_off"][-1] - 1)}, {"ver_off": a["ver_off"] + 1}, {"st_off": a["st_off"] + 1},
        {"ent_off": a["ent_off"][::-1].copy()}, {"n_versions": 0}, {"n_reasons": 2}, {"reason_check_clusters": 0},
        {"reason_check_clusters": 2}, {"reason_ns_not_federated": a["n_reasons"]}, {"n_clusters": -1},
        {"n_clusters": int(a["ent_cluster"].max())},
    ]
    for change in bad:
        assert fin_check(runtime, {**a, **change}) == runtime.KAD_EINVAL, change
    assert fin_check(runtime, {**a, "n_clusters": 16384}) == 0
    assert fin_check(runtime, {**a, "n_clusters": 16385}) == runtime.KAD_EUNSUPPORTED
    head, rest = split(a, FIN_HEAD)
    b, v, _keep, _out = runtime.sync_finish_args(*head, **rest)
    v.obj_out = None
    assert runtime._check("sync_finish", (b, v)) == runtime.KAD_EINVAL
    empty = SC.pack(SC.names(3), []).finish_arrays()
    assert fin_check(runtime, empty) == 0


def test_needs_update_validation(runtime):
    cl, objects, rows = SC.update_rows(3, 9, 10, 4)
    a = SC.pack_rows(cl, objects, rows).needs_update_arrays()
    C = a.pop("n_clusters")
    assert runtime.sync_needs_update_check(C, **a) == 0
    V, O = len(a["ver_flags"]), len(a["obj_flags"])

    def patched(key, index, value):
        x = a[key].copy()
        x[index] = value
        return {key: x}

    two = int(np.flatnonzero(np.diff(a["rec_off"]) >= 2)[0])
    lo = int(a["rec_off"][two])
    bad = [patched("rec_cluster", lo + 1, a["rec_cluster"][lo]), patched("rec_cluster", lo, C), patched("rec_cluster", lo, -1),
           patched("rec_version", 0, V), patched("rec_version", 0, -1), patched("row_obj", 0, O), patched("row_obj", 0, -1),
           patched("row_cluster", 0, C), patched("row_target", 0, V), patched("row_flags", 0, 16), patched("obj_flags", 0, 2),
           patched("ver_flags", 0, 2), patched("ver_flags", 1, 8), {"n_versions": 0}, {"rec_off": a["rec_off"][::-1].copy()}]
    for change in bad:
        assert runtime.sync_needs_update_check(C, **{**a, **change}) == runtime.KAD_EINVAL, change
    assert runtime.sync_needs_update_check(-1, **a) == runtime.KAD_EINVAL
    assert runtime.sync_needs_update_check(16385, **a) == runtime.KAD_EUNSUPPORTED
    b, v, _keep, _out = runtime.sync_needs_update_args(C, **a)
    v.recorded = None
    assert runtime._check("sync_needs_update", (b, v)) == runtime.KAD_EINVAL


def test_routes(runtime):
    ev = runtime.sync_finish_route_eval
    long_min = ev(1, 0, 1)["long_min"]
    assert long_min == 512
    per_lane = 2
    for width in (1, 2, 4, 8, 16, 32, 64):  # the width boundaries: a mean of per_lane * width entries, and one more
        assert ev(1000, 0, 1000 * per_lane * width)["width"] == width
        assert ev(1000, 0, 1000 * per_lane * width + 1)["width"] == min(64, 2 * width)
    assert ev(1000, 0, 0)["width"] == 1 and ev(1000, 0, 10 ** 9)["width"] == 64
    r = ev(1000, 10, 990 * 64)
    assert r == {"width": 32, "long_min": long_min, "threads": 256, "grid": 125, "long_grid": 10, "stride": 125 * 8}
    assert ev(5, 5, 0)["grid"] == 0 and ev(5, 5, 0)["long_grid"] == 5 and ev(0, 0, 0)["grid"] == 0
    assert ev(10 ** 6, 0, 10 ** 6, 4) == {"width": 1, "long_min": long_min, "threads": 256, "grid": 32, "long_grid": 0, "stride": 32 * 256}
    for args in ((-1, 0, 0), (1, 2, 0), (1, 0, -1), (1, 0, 0, 0)):
        with pytest.raises(runtime.KadError) as e:
            ev(*args)
        assert e.value.code == runtime.KAD_EINVAL
    nu = runtime.sync_needs_update_route_eval
    assert nu(0)["grid"] == 0 and nu(1)["grid"] == 1 and nu(256)["grid"] == 1 and nu(257) == {"threads": 256, "grid": 2, "stride": 512}
    assert nu(10 ** 7)["grid"] == 2048 and nu(10 ** 7, 4)["grid"] == 32
    with pytest.raises(runtime.KadError):
        nu(-1)


def test_declared(runtime):
    declared = {n for n in runtime.declared_functions() if n.startswith("kad_sync_")}
    assert declared == {"kad_sync_" + c + s for c in ("needs_update", "finish")
                        for s in ("", "_check", "_timing", "_route_eval", "_last_route")} | {"kad_sync_finish_debug_route"}
