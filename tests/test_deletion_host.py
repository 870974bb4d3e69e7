"""Sync deletion on the host alone: kad_deletion_decide, deletion.plan_numpy / finish_numpy, both kad_*_check
validations, route_deletion and the packer (deletion.DeletionBatch) against deletion_ref.py, the per-object restatement
of the reference's control flow; and tests/deletion_main.cpp, a program of its own built with the host code under
AddressSanitizer and UndefinedBehaviorSanitizer. Nothing here needs a GPU, and nothing sanitized is loaded into Python."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import deletion_cases as DC
import deletion_ref as R
from kubeadmiral_amd import deletion as DL
from kubeadmiral_amd import dispatch as DI
from kubeadmiral_amd import synth

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


@pytest.fixture(scope="module")
def rt():
    from kubeadmiral_amd import build, runtime
    build.build()
    return runtime


def test_decide_over_the_truth_table(rt):
    seen = set()
    for arm in DC.ARMS:
        for ready in (True, False):
            for name, ob in DC.OBSERVATIONS.items():
                op, rem, failed = R.decide(DC.fed_of(arm), ready, ob)
                got = rt.deletion_decide(DC.obj_flags_of(DC.fed_of(arm)), ready, DC.ob_flags_of(ob))
                assert got == (DC.OP[op], rem, failed), (arm, ready, name)
                seen.add(got)
    assert seen == {(0, False, False), (0, False, True), (3, True, False), (4, True, False), (4, False, False)}
    for bad in ((16, 1, 1), (1, 1, 16)):
        with pytest.raises(rt.KadError) as e:
            rt.deletion_decide(*bad)
        assert e.value.code == rt.KAD_EINVAL


def _numpy_equals_ref(worlds, clusters, clusters2=None):
    arr = DC.pack(worlds, clusters, clusters2)
    want, traces = DC.want_of(worlds, clusters, clusters2)
    assert DC.same(DL.plan_numpy(**DC.plan_args(arr)), want, DC.PLAN_OUT) is None
    assert DC.same(DL.finish_numpy(**arr), want, DC.FINISH_OUT) is None
    return arr, want, traces


def test_numpy_restatements_against_the_reference():
    for worlds, clusters in DC.truth_batches():
        _numpy_equals_ref(worlds, clusters)
    reasons = set()
    for seed, unready, unready2 in ((1, (), ()), (2, (7,), (7,)), (3, (), (0, 256)), (4, (), ())):
        worlds, clusters = DC.random_worlds(seed, 400, 257, unready=unready)
        ready2 = np.ones(257, bool)
        ready2[list(unready2)] = False
        _, want, _ = _numpy_equals_ref(worlds, clusters, DC.clusters_of(ready2))
        reasons |= set(want["obj_reason"].tolist())
    assert reasons == set(range(9))


def test_reason_precedence():
    for worlds, clusters, clusters2, reasons in DC.precedence_worlds():
        arr, want, traces = _numpy_equals_ref(worlds, clusters, clusters2)
        assert [t.reason for _, t in traces] == reasons
        assert [DC.REASONS[r] for r in DL.finish_numpy(**arr)["obj_reason"]] == reasons


def _good():
    worlds, clusters = DC.random_worlds(5, 40, 33, max_members=5)
    worlds[0]["checks"] = {"c00003": "labelled", "c00009": "deleting"}
    worlds[1]["members"] = {"c00002": DC.OBSERVATIONS["exists"], "c00020": DC.OBSERVATIONS["failed"]}
    return DC.pack(worlds, clusters)


def _edit(arr, **changes):
    out = {k: np.array(v, copy=True) for k, v in arr.items()}
    for k, f in changes.items():
        out[k] = f(out[k]) if callable(f) else f
    return out


def _set(i, v):
    def f(a):
        a[i] = v
        return a
    return f


PLAN_RULES = {
    "cluster flag unknown": dict(cluster_flags=_set(32, 16)),
    "object flag unknown": dict(obj_flags=_set(39, 16)),
    "orphan all with orphan adopted": dict(obj_flags=_set(3, 1 | 2 | 4)),
    "possible orphan with the finalizer": dict(obj_flags=_set(3, 8 | 1)),
    "possible orphan with an orphan flag": dict(obj_flags=_set(3, 8 | 4)),
    "offsets not from 0": dict(obj_ob_off=_set(0, 1)),
    "offsets decrease": dict(obj_ob_off=lambda a: _set(2, int(a[1]) - 1)(a) if a[1] > 0 else _set(1, 1)(_set(2, 0)(a))),
    "id negative": dict(ob_cluster=_set(0, -1)),
    "id at n_clusters": dict(ob_cluster=_set(-1, 33)),
    "ids equal within an object": dict(obj_flags=np.array([1], np.uint8), obj_ob_off=np.array([0, 2], np.int32),
                                       ob_cluster=np.array([4, 4], np.int32), ob_flags=np.array([1, 1], np.uint8),
                                       op_ok=np.array([1, 1], np.uint8), obj_wait=np.zeros(1, np.uint8), chk_off=np.zeros(2, np.int32),
                                       chk_cluster=np.zeros(0, np.int32), chk_flags=np.zeros(0, np.uint8)),
    "ids descend within an object": dict(obj_flags=np.array([1], np.uint8), obj_ob_off=np.array([0, 2], np.int32),
                                         ob_cluster=np.array([5, 4], np.int32), ob_flags=np.array([1, 1], np.uint8),
                                         op_ok=np.array([1, 1], np.uint8), obj_wait=np.zeros(1, np.uint8), chk_off=np.zeros(2, np.int32),
                                         chk_cluster=np.zeros(0, np.int32), chk_flags=np.zeros(0, np.uint8)),
    "observation flag unknown": dict(ob_flags=_set(0, 17)),
    "exists with retrieval failed": dict(ob_flags=_set(0, 9)),
    "an observation that says nothing": dict(ob_flags=_set(0, 0)),
    "deleting without exists": dict(ob_flags=_set(0, 8 | 2)),
    "adopted without exists": dict(ob_flags=_set(0, 8 | 4)),
}
FINISH_RULES = {
    "op_ok other than 0 and 1": dict(op_ok=_set(-1, 2)),
    "op_ok missing": dict(op_ok=np.zeros(0, np.uint8)),
    "wait flag unknown": dict(obj_wait=_set(0, 4)),
    "check cluster flag unknown": dict(chk_cluster_flags=_set(0, 64)),
    "check offsets not from 0": dict(chk_off=_set(0, 1)),
    "check offsets decrease": dict(chk_off=lambda a: _set(1, 2)(_set(2, 1)(a))),
    "check id at n_clusters": dict(chk_cluster=_set(0, 33)),
    "check ids not ascending": dict(chk_cluster=lambda a: _set(1, int(a[0]))(a)),
    "check answer none": dict(chk_flags=_set(0, 0)),
    "check answer two": dict(chk_flags=_set(0, 4 | 8)),
    "check answer unknown": dict(chk_flags=_set(0, 16)),
}


def test_good_batch_passes_both_checks(rt):
    arr = _good()
    assert rt.deletion_check(**DC.plan_args(arr)) == 0 and rt.deletion_finish_check(**arr) == 0
    assert int(arr["chk_off"][1]) == 2  # (the rules below edit the first object's two check rows)
    none = DC.pack([], DC.clusters_of([True] * 3))
    assert rt.deletion_check(**DC.plan_args(none)) == 0 and rt.deletion_finish_check(**none) == 0
    assert rt.deletion_check(**DC.plan_args(DC.pack([DC.world("delete")], []))) == 0  # no clusters at all


@pytest.mark.parametrize("rule", sorted(PLAN_RULES))
def test_every_plan_rule_is_rejected_by_both_checks(rt, rule):
    arr = _edit(_good(), **PLAN_RULES[rule])
    assert rt.deletion_check(**DC.plan_args(arr)) == rt.KAD_EINVAL
    assert rt.deletion_finish_check(**arr) == rt.KAD_EINVAL


@pytest.mark.parametrize("rule", sorted(FINISH_RULES))
def test_every_finish_rule_is_rejected(rt, rule):
    arr = _edit(_good(), **FINISH_RULES[rule])
    assert rt.deletion_check(**DC.plan_args(arr)) == 0
    assert rt.deletion_finish_check(**arr) == rt.KAD_EINVAL


def test_counts_and_limits(rt):
    arr = _good()
    assert rt.deletion_check(**DC.plan_args(arr), n_clusters=-1) == rt.KAD_EINVAL
    assert rt.deletion_check(**DC.plan_args(arr), n_clusters=16385) == rt.KAD_EUNSUPPORTED
    assert rt.deletion_finish_check(**arr, n_clusters=16385) == rt.KAD_EUNSUPPORTED
    big = DC.pack([DC.world("delete", {"c16383": DC.OBSERVATIONS["exists"]})], DC.clusters_of([True] * 16384))
    assert rt.deletion_check(**DC.plan_args(big)) == 0 and rt.deletion_finish_check(**big) == 0
    with pytest.raises(rt.KadError) as e:
        rt.deletion_route_eval(16385, 1, 0, 0)
    assert e.value.code == rt.KAD_EUNSUPPORTED
    for bad in ((-1, 1, 0, 0), (1, -1, 0, 0), (1, 1, 2, 0), (1, 1, 0, -1)):
        with pytest.raises(rt.KadError) as e:
            rt.deletion_finish_route_eval(*bad)
        assert e.value.code == rt.KAD_EINVAL


def test_result_arrays_shorter_than_the_counts_never_reach_the_library(rt):
    arr = _good()
    for k in ("chk_cluster_flags", "op_ok", "obj_wait"):
        with pytest.raises(ValueError):
            rt.deletion_finish_check(**dict(arr, **{k: arr[k][:-1]}))


def _route(C, O, n_long, short_items, n_cu, per_lane=4, long_min=256):
    """route_deletion restated: csrc/kad_groups.h's rule with this call's constants."""
    n_short = O - n_long
    mean = -(-short_items // n_short) if n_short > 0 else 0
    want = -(-mean // per_lane)
    width = 1
    while width < 64 and width < want:
        width *= 2
    per_block = 256 // width
    grid = min(-(-O // per_block), n_cu * 8) if n_short > 0 else 0
    return dict(width=width, long_min=long_min, threads=256, grid=grid, long_grid=(n_long + 3) // 4,
                stride=grid * per_block, lds=(C + 15) // 16 * 16)


def test_route_across_the_width_and_long_boundaries(rt):
    assert rt.DELETION_ROUTE == ("width", "long_min", "threads", "grid", "long_grid", "stride", "lds")
    widths = set()
    for O in (1, 63, 64, 65, 1000, 2048 * 256 + 1):
        for mean in (0, 1, 4, 5, 8, 9, 16, 17, 32, 33, 64, 65, 128, 129, 255, 256, 257, 1000):
            for n_long in (0, 1, 4, 5, O):
                if n_long > O:
                    continue
                for n_cu, C in ((256, 1000), (1, 0), (304, 16384), (256, 15), (256, 16), (256, 17)):
                    items = mean * (O - n_long)
                    for fn in (rt.deletion_route_eval, rt.deletion_finish_route_eval):
                        got = fn(C, O, n_long, items, n_cu)
                        assert got == _route(C, O, n_long, items, n_cu), (C, O, n_long, items, n_cu)
                    widths.add(got["width"])
    assert widths == {1, 2, 4, 8, 16, 32, 64}


# ------------------------------------------------------------------ the packer
FIN, _cluster, _fed, _member, _world_of = DC.FIN, DC.cluster_obj, DC.fed_obj, DC.member_obj, DC.world_of_objects


def _packer_case():
    clusters = [_cluster("a"), _cluster("b"), _cluster("c", ready=False), _cluster("d")]
    err = RuntimeError("lookup failed")
    objs = [
        (_fed("plain"), {"d": _member(), "a": _member(deleting=True), "c": _member(), "zz": _member()}),
        (_fed("adopt", orphan="adopted"), {"a": _member(adopted=True), "b": _member(), "d": None}),
        (_fed("all", orphan="all"), {"a": _member(), "b": _member(deleting=True)}),
        (_fed("internal-wins", orphan="all", internal="nonsense"), {"b": err}),
        (_fed("no-finalizer", finalizer=False, orphan="all"), {"a": _member()}),
        (None, {"a": _member(), "d": _member(deleting=True)}),
        (_fed("gone"), {}),
    ]
    return clusters, objs


def test_packer_on_hand_written_objects():
    clusters, objs = _packer_case()
    batch = DL.DeletionBatch(None, clusters, FIN)
    for fed, members in objs:
        batch.add(fed, members)
    a = batch.arrays()
    assert a["cluster_flags"].tolist() == [9, 9, 8, 9]
    assert a["obj_flags"].tolist() == [1, 1 | 4, 1 | 2, 1, 2, 8, 1]
    assert a["obj_ob_off"].tolist() == [0, 3, 5, 7, 8, 9, 11, 11]
    assert a["ob_cluster"].tolist() == [0, 2, 3, 0, 1, 0, 1, 1, 0, 0, 3]
    assert a["ob_flags"].tolist() == [3, 1, 1, 5, 1, 1, 3, 8, 1, 1, 3]
    ref_clusters = [("a", True), ("b", True), ("c", False), ("d", True)]
    worlds = [_world_of(f, m) for f, m in objs]
    plans = batch.apply_plan(DL.plan_numpy(**a))
    for w, p in zip(worlds, plans):
        _, t = R.reconcile(w, ref_clusters)
        assert list(p.ops.items()) == [(n, {R.DELETE: DI.OP_DELETE, R.REMOVE_LABEL: DI.OP_REMOVE_LABEL}[op]) for n, op in t.ops]
        assert (p.remaining, p.retrieval_failed, p.unready) == (t.remaining, t.retrieval_failed, t.unready)
        at = t.actions.index("ops") if "ops" in t.actions else len(t.actions)
        assert p.first == t.actions[:at]
    assert plans[0].ops == {"a": DI.OP_DELETE, "d": DI.OP_DELETE} and plans[1].ops == {"a": DI.OP_REMOVE_LABEL, "b": DI.OP_DELETE}
    assert plans[2].first == ["delete-history", "remove-finalizer"] and plans[2].ops == {"a": DI.OP_REMOVE_LABEL}
    assert plans[4].first == ["nothing"] and plans[4].unready == [] and plans[5].ops == {"a": DI.OP_REMOVE_LABEL}


def _outcomes(clusters, clusters2, ref_clusters, ref_clusters2, cases):
    """cases: (fed, members, op_results, wait bits, checks). → (the packer's outcomes, the reference's)."""
    batch = DL.DeletionBatch(None, clusters, FIN)
    for fed, members, *_ in cases:
        batch.add(fed, members)
    fa = batch.finish_arrays([c[2] for c in cases], [c[3] for c in cases], [c[4] for c in cases], clusters2)
    plans = batch.apply_plan(DL.plan_numpy(**batch.arrays()))
    got = batch.apply_finish(DL.finish_numpy(**fa), plans, clusters2)
    want = []
    for fed, members, ops, wait, checks in cases:
        w = _world_of(fed, members)
        w["op_ok"] = dict(ops)
        w["wait_timed_out"], w["check_timed_out"] = bool(wait & 1), bool(wait & 2)
        for n, m in checks.items():
            w["checks"][n] = ("get_failed" if isinstance(m, Exception) else "deleting" if "deletionTimestamp" in m["metadata"]
                              else "labelled" if m["metadata"]["labels"].get(DL.MANAGED_LABEL) == "true" else "unlabelled")
        want.append(R.reconcile(w, ref_clusters, ref_clusters2))
    return got, want


def test_go_error_strings_and_outcomes():
    ready = [_cluster("a"), _cluster("b"), _cluster("c"), _cluster("d")]
    c_down = [_cluster("a"), _cluster("b"), _cluster("c", ready=False), _cluster("d", ready=False)]
    r_ready, r_down = [(n, True) for n in "abcd"], [("a", True), ("b", True), ("c", False), ("d", False)]
    err = RuntimeError("boom")
    first_down = [
        (_fed("x"), {"a": _member(), "b": _member()}, {}, 1, {}),
        (_fed("y"), {"a": err, "b": err}, {}, 0, {}),
        (_fed("z"), {"a": _member()}, {"a": False}, 0, {}),
        (None, {"a": _member()}, {}, 0, {}),
    ]
    got, want = _outcomes(c_down, None, r_down, None, first_down)
    texts = ["Failed to finish 2 operations in 30s",
             "failed to retrieve a managed resource for the following cluster(s): a, b",
             "the following clusters were not ready: c, d", "the following clusters were not ready: c, d"]
    second_down = [
        (_fed("p"), {"a": _member()}, {"a": False}, 0, {}),
        (_fed("q", orphan="all"), {"a": _member()}, {"a": False}, 0, {}),
        (None, {"b": _member()}, {"b": False}, 0, {}),
        (_fed("r"), {"a": _member()}, {}, 2, {}),
        (_fed("s"), {}, {}, 2, {}),
        (_fed("t"), {}, {}, 0, {"a": _member()}),
        (_fed("u", orphan="all"), {"a": _member()}, {}, 0, {}),
    ]
    g2, w2 = _outcomes(ready, c_down, r_ready, r_down, second_down)
    verify = "failed to verify that managed resources no longer exist in any cluster: "
    texts += ["failed to remove managed resources from one or more clusters.",
              "failed to remove the label from resources in one or more clusters.",
              "failed to remove the label from resources in one or more clusters.", None,
              verify + "Failed to finish 2 operations in 30s", verify + "the following clusters were not ready: c, d", None]
    all_ready = [
        (_fed("v"), {}, {}, 0, {"a": _member(), "c": err}),
        (_fed("w"), {}, {}, 0, {"a": _member(labelled=False)}),
        (_fed("nf", finalizer=False), {"a": _member()}, {}, 0, {}),
    ]
    g3, w3 = _outcomes(ready, None, r_ready, None, all_ready)
    texts += [verify + "one or more checks failed", None, None]
    got, want = got + g2 + g3, want + w2 + w3
    assert [o.error for o in got] == texts
    for o, (result, t) in zip(got, want):
        assert (o.result, o.reason, o.error, o.recorded_error) == (result, t.reason, t.error, t.recorded_error)
        at = t.actions.index("ops") if "ops" in t.actions else len(t.actions)
        assert o.then == t.actions[at + 1:]
    assert got[0].recorded_error == 'failed to delete FederatedDeployment "ns/x": Failed to finish 2 operations in 30s'
    assert got[3].recorded_error is None and got[5].recorded_error is None  # the label arms only return the error
    assert [o.result for o in got] == ["Error"] * 7 + ["Recheck", "Error", "Error", "OK", "Error", "OK", "OK"]
    assert got[-2].then == ["delete-history", "remove-finalizer"] and got[-1].then == []


def test_gen_deletion_is_valid_and_varied(rt):
    arr = synth.gen_deletion(7, 3000, 1000)
    assert rt.deletion_finish_check(**arr) == 0
    assert tuple(arr)[:5] == synth.DELETION_PLAN_KEYS == DC.PLAN_KEYS
    n = np.diff(arr["obj_ob_off"])
    assert 9 <= n[n > 0].mean() <= 11 and 0.15 < (n == 0).mean() < 0.25
    fin = DL.finish_numpy(**arr)
    assert set(fin["obj_reason"].tolist()) >= {0, 1, 2, 4, 5, 6, 8} and set(fin["obj_status"].tolist()) == {0, 1, 2}
    shaky = synth.gen_deletion(7, 300, 1000, healthy=0.99)
    assert rt.deletion_finish_check(**shaky) == 0 and set(DL.finish_numpy(**shaky)["obj_reason"].tolist()) & {3, 7}


def test_stand_alone_program_under_sanitizers(tmp_path):
    """tests/deletion_main.cpp with csrc/kad_deletion.hip: the host code under ASan + UBSan, run as its own process."""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not os.path.exists(hipcc):
        hipcc = shutil.which("hipcc")
    if hipcc is None:
        pytest.fail("no hipcc")
    exe = str(tmp_path / "deletion_main")
    san = ["-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=all", "-Xarch_host",
           "-fno-omit-frame-pointer"]
    subprocess.run([hipcc, "--offload-arch=" + os.environ.get("KAD_OFFLOAD_ARCH", "gfx950"), "-std=c++17", "-O1", "-g", *san, "-pthread", os.path.join(HERE, "deletion_main.cpp"),
                    os.path.join(ROOT, "kubeadmiral_amd", "csrc", "kad_deletion.hip"), "-o", exe], check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="halt_on_error=1")
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, env=env, timeout=300)
    out = r.stdout.decode(errors="replace")
    assert r.returncode == 0, out
    assert out.startswith("ok: "), out
