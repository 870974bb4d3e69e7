"""kad_dispatch_plan without a GPU: the numpy restatement and the shared decision function against the
cluster-by-cluster checker (dispatch_ref.py), the library's validation and launch decision, and the packer on
hand-written objects."""
import numpy as np
import pytest

import dispatch_cases as DC
import dispatch_ref as R
from kubeadmiral_amd import dispatch as DI
from kubeadmiral_amd import objects as O
from kubeadmiral_amd import synth

BATCHES = [("truth",)] + [("shapes", C) for C in DC.SHAPE_CS] + \
    [("random", n, 257, 3) for n in (1, 3, 4, 5, 63, 64, 65)] + [("tiny", 4 * 2048 + 1), ("synth", 9, 600, 257)]


@pytest.fixture(scope="module")
def runtime():
    from kubeadmiral_amd import build, runtime
    build.build()
    return runtime


@pytest.mark.parametrize("key", BATCHES, ids=lambda k: "-".join(map(str, k)))
def test_plan_numpy_equals_the_checker(key):
    arr, want = DC.case(*key)
    assert DC.entries_equal(DI.plan_numpy(fill=DC.FILL, **arr), want, arr["out_off"], DC.FILL) is None


def test_decision_function_equals_the_checker(runtime):
    """di_decide, the function the kernel calls, on the whole truth table, one pair at a time."""
    arr, combos = DC.truth_table()
    seen = set()
    for (sel, ob, orphan), cf in ((c, f) for c in combos for f in range(16)):
        recorded, n_ops, recheck = R.sync_to_clusters([("c", cf)], {"c"} if sel else set(),
                                                      {"c": "error" if ob == R.RETRIEVAL_FAILED else ob},
                                                      {0: "", R.ORPHAN_ALL: "all", R.ORPHAN_ADOPTED: "adopted"}[orphan])
        want = (recorded[0][1], R.ST[recorded[0][2]], recheck) if recorded else (R.NONE, 0, False)
        assert runtime.dispatch_decide(cf, sel, ob or 0, orphan) == want, (cf, sel, ob, orphan)
        seen.add(want)
    assert {s for _, s, _ in seen} == set(range(10)) and {o for o, _, _ in seen} == set(range(5))
    assert (R.NONE, R.ST["FinalizerCheckFailed"], True) in seen


def test_the_synthetic_batch_is_mostly_creates_and_updates():
    """The condition on synth.gen_dispatch the GPU test relies on, confirmed with the checker."""
    arr, want = DC.case("synth", 9, 600, 257)
    live = np.concatenate([np.arange(o, o + c) for o, c in zip(arr["out_off"][:-1], want["count"])]).astype(np.int64)
    ops = np.array(want["out_op"])[live]
    assert len(ops) > 2000 and np.isin(ops, (R.CREATE, R.UPDATE)).mean() >= 0.8
    assert len(set(np.array(want["out_status"])[live].tolist())) == 9 and (np.array(want["obj_result"]) == R.RECHECK).any()


def _bad(arr, **change):
    a = dict(arr)
    for k, v in change.items():
        a[k] = v(np.array(a[k])) if callable(v) else v
    return a


def _set(i, v):
    def f(a):
        a[i] = v
        return a
    return f


def test_check_rejects_every_invalid_input(runtime):
    arr, _ = DC.case("random", 65, 257, 3)
    assert runtime.dispatch_check(**arr) == 0
    ob_at = int(np.flatnonzero(np.diff(arr["obj_ob_off"]) >= 2)[0])
    k = int(arr["obj_ob_off"][ob_at])
    need = np.diff(arr["obj_pl_off"]) + np.diff(arr["obj_ob_off"])
    exact = int(np.flatnonzero((need >= 1) & (np.diff(arr["out_off"]) == need))[0])  # an object without slack

    def swap(a):
        a[k], a[k + 1] = a[k + 1], a[k]
        return a
    bads = {
        "pl_off decreases": _bad(arr, obj_pl_off=_set(3, int(arr["obj_pl_off"][-1]) + 1)),
        "pl_off from 1": _bad(arr, obj_pl_off=_set(0, 1)),
        "ob_off decreases": _bad(arr, obj_ob_off=_set(ob_at + 1, k - 1 if k else -1)),
        "ns_off from 5": _bad(arr, ns_pl_off=_set(0, 5)),
        "ns_off decreases": _bad(arr, ns_pl_off=_set(1, -1)),
        "out_off decreases": _bad(arr, out_off=_set(2, -1)),
        "pl id C": _bad(arr, pl_cluster=_set(0, 257)),
        "pl id -2": _bad(arr, pl_cluster=_set(0, -2)),
        "ns id C": _bad(arr, ns_cluster=_set(0, 257)),
        "ob id C": _bad(arr, ob_cluster=_set(int(arr["obj_ob_off"][ob_at + 1]) - 1, 257)),
        "ob id -1": _bad(arr, ob_cluster=_set(k, -1)),
        "ob equal": _bad(arr, ob_cluster=_set(k + 1, int(arr["ob_cluster"][k]))),
        "ob descending": _bad(arr, ob_cluster=swap),
        "cluster flag 16": _bad(arr, cluster_flags=_set(0, 16)),
        "obj flag 8": _bad(arr, obj_flags=_set(0, 8)),
        "both orphan modes": _bad(arr, obj_flags=_set(0, R.ORPHAN_ALL | R.ORPHAN_ADOPTED)),
        "ob flag 16": _bad(arr, ob_flags=_set(0, 16 | R.EXISTS)),
        "deleting without exists": _bad(arr, ob_flags=_set(0, R.DELETING)),
        "adopted without exists": _bad(arr, ob_flags=_set(0, R.ADOPTED | R.RETRIEVAL_FAILED)),
        "failed and exists": _bad(arr, ob_flags=_set(0, R.EXISTS | R.RETRIEVAL_FAILED)),
        "no flag at all": _bad(arr, ob_flags=_set(0, 0)),
        "obj_ns N": _bad(arr, obj_ns=_set(0, 1)),
        "obj_ns -3": _bad(arr, obj_ns=_set(0, -3)),
        "capacity below the bound": _bad(arr, out_off=lambda a: np.concatenate((a[:exact + 1], a[exact + 1:] - 1))),
    }
    for name, a in bads.items():
        assert runtime.dispatch_check(**a) == runtime.KAD_EINVAL, name
    # the bound itself is enough
    tight = DC.pack([DC.HEALTHY] * 4, [DC.obj(pl=[0, 1, 1], ob=[(2, R.EXISTS)])])
    assert tight["out_off"].tolist() == [0, 4] and runtime.dispatch_check(**tight) == 0


def test_check_refuses_more_clusters_than_the_wave_path_holds(runtime):
    top = DC.pack([DC.HEALTHY] * 16384, [DC.obj(pl=[16383], ob=[(16383, R.EXISTS)])])
    assert runtime.dispatch_check(**top) == 0
    over = DC.pack([DC.HEALTHY] * 16385, [DC.obj(pl=[16384], ob=[(16384, R.EXISTS)])])
    assert runtime.dispatch_check(**over) == runtime.KAD_EUNSUPPORTED
    with pytest.raises(runtime.KadError) as e:
        runtime.dispatch_route_eval(16385, 1)
    assert e.value.code == runtime.KAD_EUNSUPPORTED
    with pytest.raises(ValueError):
        DI.DispatchBatch(O.FederatedTypeConfig(), [{"metadata": {"name": f"c{i}"}} for i in range(16385)], "f")


def test_route(runtime):
    for C, words in ((1, 1), (32, 1), (33, 2), (16384, 512)):
        r = runtime.dispatch_route_eval(C, 1000, 256)
        assert (r["words"], r["threads"], r["lds"]) == (words, 256, 4 * 3 * words * 4)
        assert r["grid"] == 250 and r["stride"] == 1000
    for n, grid in ((0, 0), (1, 1), (4, 1), (5, 2)):
        r = runtime.dispatch_route_eval(1000, n, 256)
        assert (r["grid"], r["stride"]) == (grid, 4 * grid)
    # more objects than the grid covers: as many blocks as stay resident, the waves stride
    r = runtime.dispatch_route_eval(1000, 10_000_000, 256)
    assert r["grid"] == 256 * 8 and r["stride"] == 4 * r["grid"]
    r = runtime.dispatch_route_eval(16384, 10_000_000, 256)
    assert r["lds"] == 24576 and r["grid"] == 256 * 6 and r["stride"] == 4 * r["grid"]


FIN = DI.cascading_delete_finalizer("deployments.apps")


def _cluster(name, ready=True, terminating=False, cascading=False, finalizer=True):
    c = {"metadata": {"name": name, "finalizers": ["other"] + ([FIN] if finalizer else [])},
         "status": {"conditions": [{"type": "Joined", "status": "True"}, {"type": "Ready", "status": "True" if ready else "False"}]}}
    if terminating:
        c["metadata"]["deletionTimestamp"] = "2024-01-01T00:00:00Z"
    if cascading:
        c["metadata"]["annotations"] = {DI.CASCADING_DELETE_ANNOTATION: ""}
    return c


def _fed(name, placements, namespace="default", annotations=None):
    return {"apiVersion": "types.kubeadmiral.io/v1alpha1", "kind": "FederatedDeployment",
            "metadata": {"name": name, "namespace": namespace, "annotations": annotations or {}},
            "spec": {"placements": [{"controller": c, "placement": {"clusters": [{"name": n} for n in names]}}
                                    for c, names in placements]}}


def test_finalizer_and_cluster_flags():
    assert DI._fnv32(b"") == 2166136261 and DI._fnv32(b"a") == 0x050C5D7E  # FNV-1, not FNV-1a
    assert FIN == f"kubeadmiral.io/cascading-delete-deployments.apps-{DI._fnv32(b'deployments.apps')}"
    assert DI.cascading_delete_finalizer("x" * 30).startswith("kubeadmiral.io/cascading-delete-" + "x" * 20 + "-")
    assert DI.cluster_flags_of(_cluster("a"), FIN) == R.READY | R.FINALIZER
    assert DI.cluster_flags_of(_cluster("a", False, True, True, False), FIN) == R.TERMINATING | R.CASCADING
    assert DI.cluster_flags_of({"metadata": {"name": "a"}}, FIN) == 0


def test_dispatch_batch_on_hand_written_objects():
    ftc = O.FederatedTypeConfig("apps", "v1", "Deployment", "deployments", "Namespaced", "spec.replicas")
    clusters = [_cluster(n) for n in ("a", "b", "c", "d")]
    fed_ns = {"default": _fed("default", [("kubeadmiral.io/nsautoprop-controller", ["d", "b", "a", "gone"])], namespace=""),
              "broken": {"metadata": {"name": "broken"}, "spec": {"placements": "no list"}}}
    lookup_error = LookupError("informer not synced")
    adopted = {"metadata": {"name": "x", "annotations": {DI.ADOPTED_ANNOTATION: "true"}}}
    deleting = {"metadata": {"name": "x", "deletionTimestamp": "2024-01-01T00:00:00Z", "annotations": {DI.ADOPTED_ANNOTATION: "false"}}}
    b = DI.DispatchBatch(ftc, clusters, FIN, fed_ns)
    # two controllers' placements with a shared cluster, a name that is not joined
    b.add(_fed("one", [("kubeadmiral.io/global-scheduler", ["c", "a"]), ("kubeadmiral.io/follower-controller", ["a", "zz", "b"])]),
          {"a": adopted, "c": lookup_error, "b": None, "zz": adopted, "d": deleting})
    b.add(_fed("two", [("s", ["a"])], namespace="elsewhere"), {})                                   # no federated namespace
    b.add(_fed("three", [("s", ["a"])], annotations={DI.ORPHAN_ANNOTATION: "all", DI.ORPHAN_INTERNAL_ANNOTATION: "adopted"}), {})
    b.add(_fed("four", [("s", ["a"])], annotations={DI.ORPHAN_ANNOTATION: "all", DI.ORPHAN_INTERNAL_ANNOTATION: "nonsense"}), {})
    b.add(_fed("five", [("s", ["a"])], annotations={DI.ORPHAN_ANNOTATION: "all"}), {})
    b.add({"metadata": {"name": "six", "namespace": "default"}, "spec": {"placements": [{"placement": {"clusters": "x"}}]}}, {"a": adopted})
    b.add(_fed("seven", [("s", ["a"])], namespace="broken"), {})
    a = b.arrays()
    assert a["cluster_flags"].tolist() == [R.READY | R.FINALIZER] * 4
    assert a["obj_pl_off"].tolist() == [0, 5, 6, 7, 8, 9, 9, 10] and a["pl_cluster"][:5].tolist() == [2, 0, 0, -1, 1]
    assert a["ns_pl_off"].tolist() == [0, 4] and a["ns_cluster"].tolist() == [3, 1, 0, -1]
    assert a["obj_ns"].tolist() == [0, -2, 0, 0, 0, -1, -1]
    assert a["obj_flags"].tolist() == [0, 0, R.ORPHAN_ADOPTED, 0, R.ORPHAN_ALL, R.ERROR, R.ERROR]
    assert a["obj_ob_off"].tolist() == [0, 3, 3, 3, 3, 3, 4, 4] and a["ob_cluster"].tolist() == [0, 2, 3, 0]
    assert a["ob_flags"].tolist() == [R.EXISTS | R.ADOPTED, R.RETRIEVAL_FAILED, R.EXISTS | R.DELETING, R.EXISTS | R.ADOPTED]
    assert a["out_off"].tolist() == [0, 8, 9, 10, 11, 12, 13, 14]  # placement entries plus observations, no less
    assert b.errors[5] and "broken" in b.errors[6]
    from kubeadmiral_amd import runtime  # the packed batch passes the library's validation where it is built
    import os
    if os.path.exists(runtime.LIB_PATH):
        assert runtime.dispatch_check(**a) == 0
    out = b.apply(DI.plan_numpy(**a))
    one = out[0]
    assert one.selected == {"a", "b"} and one.ops == {"a": R.UPDATE, "b": R.CREATE}
    assert one.status == {"a": "UpdateTimedOut", "b": "CreationTimedOut", "c": "CachedRetrievalFailed", "d": "WaitingForRemoval"}
    assert one.to_delete == set() and not one.recheck and one.reason is None
    assert one.rollout_members == {"a": adopted, "b": None, "d": deleting}
    assert out[1].selected == set() and not out[1].ops and not out[1].status
    assert out[5].reason == out[6].reason == "ComputePlacementFailed" and not out[5].status
    # the three obj_ns cases of a namespaced type, and a cluster-scoped one
    limited = DI.DispatchBatch(ftc, clusters, FIN, fed_ns, limited_scope=True)
    limited.add(_fed("two", [("s", ["a"])], namespace="elsewhere"), {})
    limited.add(_fed("one", [("s", ["a", "c"])]), {})
    assert limited.arrays()["obj_ns"].tolist() == [-1, 0]
    assert [o.selected for o in limited.apply(DI.plan_numpy(**limited.arrays()))] == [{"a"}, {"a"}]
    scoped = DI.DispatchBatch(O.FederatedTypeConfig("", "v1", "Namespace", "namespaces", "Cluster"), clusters, FIN, fed_ns)
    scoped.add(_fed("default", [("s", ["c"])], namespace=""), {})
    assert scoped.arrays()["obj_ns"].tolist() == [-1]


def test_outcomes_of_unhealthy_clusters():
    """One object over a not-ready, a cascading, a terminating and a finalizer-less cluster."""
    ftc = O.FederatedTypeConfig("apps", "v1", "Deployment", "deployments", "Cluster")
    clusters = [_cluster("ok"), _cluster("down", ready=False), _cluster("casc", terminating=True, cascading=True),
                _cluster("term", terminating=True), _cluster("nofin", finalizer=False), _cluster("left")]
    member = {"metadata": {"name": "x"}}
    b = DI.DispatchBatch(ftc, clusters, FIN)
    b.add(_fed("x", [("s", ["ok", "down", "casc", "term", "nofin"])], annotations={DI.ORPHAN_ANNOTATION: "all"}),
          {"ok": member, "casc": member, "term": member, "left": member, "down": member})
    o = b.apply(DI.plan_numpy(**b.arrays()))[0]
    assert o.ops == {"ok": R.UPDATE, "casc": R.REMOVE_LABEL, "left": R.DELETE} and o.to_delete == {"casc", "left"}
    assert o.status == {"ok": "UpdateTimedOut", "down": "ClusterNotReady", "casc": "LabelRemovalTimedOut",
                        "term": "ClusterTerminating", "nofin": "FinalizerCheckFailed", "left": "DeletionTimedOut"}
    assert o.recheck and o.selected == {"ok", "down", "casc", "term", "nofin"}
    assert set(o.rollout_members) == {"ok", "casc", "term", "nofin", "left"}
