"""Revision history on the host: the per-object reference against the written cases, the packing and its CPU
restatement against the reference, kad_revision_plan_check's every error row, the route at its boundaries, and the
shared header's host functions in a stand-alone program under the host sanitizers."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import history_cases as HC
import history_ref as R
from kubeadmiral_amd import gojson, history as H, synth

HERE = os.path.dirname(os.path.abspath(__file__))
_NAMED = HC.named()


@pytest.fixture(scope="module")
def rt():
    from kubeadmiral_amd import build, runtime
    build.build()
    return runtime


def want_of(entry, actions, last):
    got = R.sync_revisions(entry)
    if actions is None:
        return ("Error", entry["error"], [], entry["collision"], "", "")
    new = got[5]
    return ("AllOK", None, [(k, new if n == HC.NEW else n, v) for k, n, v in actions], entry["collision"], last,
            "" if entry["limit"] == 0 else new)


def test_fnv_and_alphabet_vectors():
    # FNV-1 32 test vectors of the FNV reference distribution; the alphabet byte by byte
    assert R.fnv1_32(b"") == 0x811C9DC5 and R.fnv1_32(b"a") == 0x050C5D7E and R.fnv1_32(b"foobar") == 0x31F0B262
    assert R.safe_encode_string("0123456789") == "456789bcdf" == H.safe_encode("0123456789")
    assert R.hash_controller_revision(b"a", None) == R.safe_encode_string(str(0x050C5D7E)) == "d8bfb88b"  # 84696446
    # "a" then the probe "-12": three more FNV steps
    h = 0x050C5D7E
    for ch in b"-12":
        h = (h * 16777619) % 2 ** 32 ^ ch
    assert R.hash_controller_revision(b"a", -12) == R.safe_encode_string(str(h))
    assert R.controller_revision_name("p" * 300, "x") == "p" * 223 + "-x" == H.revision_name("p" * 300, "x")
    for s, v in [("12", 12), ("+12", 12), ("-12", -12), ("2147483647", 2147483647), ("2147483648", None), ("-2147483648", -2147483648),
                 ("", None), ("+", None), ("1_0", None), ("0x1", None), (" 1", None), ("٣", None), ("007", 7)]:
        assert R.parse_int_10_32(s) == v == H.parse_int32(s), s


def test_patch_bytes():
    tpl = {"spec": {"b": 1, "a": [1.5, True, None, "<x>"]}, "metadata": {}}
    fed = {"spec": {"template": {"spec": {"template": tpl}}}}
    assert H.get_patch(fed) == (b'[{"op":"replace","path":"/spec/template/spec/template","value":{"metadata":{},"spec":{"a":[1.5,true,null,'
                                b'"\\u003cx\\u003e"],"b":1}}}]')
    for f, s in [(1.0, "1"), (-0.0, "-0"), (1e21, "1e+21"), (1e20, "100000000000000000000"), (1e-6, "0.000001"), (1e-7, "1e-7"),
                 (1.5e-10, "1.5e-10"), (123456.789, "123456.789")]:
        assert gojson.marshal_unstructured(f) == s.encode(), f
    for bad in ({}, {"spec": {}}, {"spec": {"template": {"spec": {"template": 3}}}}, {"spec": {"template": []}}):
        with pytest.raises(H.RevisionError):
            H.get_patch(bad)


@pytest.mark.parametrize("name", sorted(_NAMED))
def test_reference_against_written_expectations(name):
    entry, actions, last = _NAMED[name]
    assert R.sync_revisions(entry) == want_of(entry, actions, last)


def test_collision_counts_change_the_name():
    names = {R.sync_revisions(_NAMED[k][0])[5] for k in ("collision_nil", "collision_0", "collision_negative", "collision_min")}
    assert len(names) == 4 and all(n.startswith("web-") for n in names)
    assert R.sync_revisions(_NAMED["long_name_prefix"][0])[5].startswith("n" * 223 + "-")


def numpy_outcomes(entries):
    b = HC.batch_of_entries(entries)
    return [R.outcome_tuple(o) for o in b.apply(H.plan_numpy(**b.arrays()))]


def test_numpy_against_reference_on_the_cases():
    entries = [e for _, (e, _, _) in sorted(_NAMED.items())]
    assert numpy_outcomes(entries) == [R.sync_revisions(e) for e in entries]
    a = HC.batch_of_entries(entries).arrays()
    assert 0 < int((a["obj_flags"] & H.OBJ_LABELS_ON_HOST != 0).sum()) < len(entries)
    assert int((a["rev_flags"] & H.REV_HASH_PARSED).sum()) >= 4


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_numpy_against_reference_on_fuzz(seed):
    entries = HC.random_objs(seed, 300)
    want = [R.sync_revisions(e) for e in entries]
    assert numpy_outcomes(entries) == want
    kinds = {k for w in want for k, _, _ in w[2]}
    assert kinds == {"create", "delete", "renumber", "relabel"}


def test_numpy_against_reference_on_gen_revisions():
    b = synth.gen_revisions(7, 400, long_every=50)
    got = [R.outcome_tuple(o) for o in b.apply(H.plan_numpy(**b.arrays()))]
    want = [R.sync_revisions(e) for e in b.objs]
    assert got == want
    quiet = sum(1 for w in want if not w[2])
    assert 0.7 * len(want) < quiet < len(want)  # most objects are in the steady state
    assert max(len(e["patch"]) for e in b.objs) > 50 * min(len(e["patch"]) for e in b.objs)


def test_update_label_agrees_with_the_string():
    """The arithmetic form of the update revision's label parse (the device's) against the characters."""
    rng = np.random.default_rng(5)
    sums = [0, 5, 6, 55555, 555555555, 1234512345, 1743039203, 1743039204, 4294967295] + rng.integers(0, 2 ** 32, 2000).tolist()
    sums += [int("".join(str(d) for d in rng.integers(0, 6, n))) for n in range(1, 10) for _ in range(50)]
    hit = 0
    for s in sums:
        v = R.parse_int_10_32(R.safe_encode_string(str(s)))
        assert H.update_label(s) == ((False, 0) if v is None else (True, v % 2 ** 32))
        hit += v is not None
    assert hit > 100


# ------------------------------------------------------------------ kad_revision_plan_check
def good():
    entries = [_NAMED[k][0] for k in ("subset_true_false_none", "old_ties_by_time_then_name", "no_revisions")]
    return HC.batch_of_entries(entries).arrays()


def test_check_accepts_the_cases_and_the_empty_batch(rt):
    assert rt.revision_plan_check(**good()) == 0
    assert rt.revision_plan_check(**HC.batch_of_entries([]).arrays()) == 0
    assert rt.revision_plan_check(**HC.batch_of_entries([e for _, (e, _, _) in sorted(_NAMED.items())]).arrays()) == 0


def _mut(key, fn):
    def f(a):
        v = a[key].copy()
        fn(v)
        a[key] = v
    return f


EINVAL_ROWS = {
    "negative n_objects": lambda a: a.update(n_objects=-1),
    "negative n_pairs": lambda a: a.update(n_pairs=-1),
    "negative blob_len": lambda a: a.update(blob_len=-1),
    "negative action_capacity": lambda a: a.update(action_capacity=-1),
    "limit missing": lambda a: a.pop("limit"),
    "collision missing": lambda a: a.pop("collision"),
    "patch_off missing": lambda a: a.pop("patch_off"),
    "patch_len missing": lambda a: a.pop("patch_len"),
    "blob missing": lambda a: a.update(blob=np.zeros(0, np.uint8), blob_len=len(a["blob"])),
    "rev_off missing": lambda a: a.pop("rev_off"),
    "rev_off not from 0": _mut("rev_off", lambda v: v.__setitem__(0, 1)),
    "rev_off decreasing": _mut("rev_off", lambda v: v.__setitem__(1, 99)),
    "rev_data_off missing": lambda a: a.pop("rev_data_off"),
    "rev_revision missing": lambda a: a.pop("rev_revision"),
    "rev_time missing": lambda a: a.pop("rev_time"),
    "rev_name_rank missing": lambda a: a.pop("rev_name_rank"),
    "rev_hash missing": lambda a: a.pop("rev_hash"),
    "obj flag unknown": _mut("obj_flags", lambda v: v.__setitem__(0, 4)),
    "patch_len negative": _mut("patch_len", lambda v: v.__setitem__(0, -1)),
    "patch_off negative": _mut("patch_off", lambda v: v.__setitem__(0, -16)),
    "patch_off unaligned": _mut("patch_off", lambda v: v.__setitem__(0, 8)),
    "patch beyond the blob": _mut("patch_off", lambda v: v.__setitem__(0, 1 << 40)),
    "patch padding beyond the blob": lambda a: a.update(blob=a["blob"][:-1]),
    "rev flag unknown": _mut("rev_flags", lambda v: v.__setitem__(0, 2)),
    "data_len negative": _mut("rev_data_len", lambda v: v.__setitem__(0, -1)),
    "data_off unaligned": _mut("rev_data_off", lambda v: v.__setitem__(0, 4)),
    "data beyond the blob": _mut("rev_data_len", lambda v: v.__setitem__(0, 1 << 30)),
    "name rank negative": _mut("rev_name_rank", lambda v: v.__setitem__(0, -1)),
    "name rank beyond the object": _mut("rev_name_rank", lambda v: v.__setitem__(0, 5)),
    "rev_lab_off missing": lambda a: a.pop("rev_lab_off"),
    "rev_lab pair beyond n_pairs": lambda a: a.update(n_pairs=1),
    "rev_lab not ascending": _mut("rev_lab", lambda v: v.__setitem__(1, v[0])),
    "want_off missing": lambda a: a.pop("want_off"),
    "want_lab negative": _mut("want_lab", lambda v: v.__setitem__(0, -1)),
    "want_lab not ascending": _mut("want_lab", lambda v: v.__setitem__(1, v[0])),
}


@pytest.mark.parametrize("row", sorted(EINVAL_ROWS))
def test_check_einval(rt, row):
    a = good()
    EINVAL_ROWS[row](a)
    assert rt.revision_plan_check(**a) == rt.KAD_EINVAL


def test_check_missing_view_and_batch(rt):
    import ctypes
    b, v, _keep, _out = rt.revision_plan_args(**good())
    L = rt.load_library()
    assert L.kad_revision_plan_check(ctypes.byref(b), None) == rt.KAD_EINVAL
    assert L.kad_revision_plan_check(None, ctypes.byref(v)) == rt.KAD_EINVAL
    for name, _ in v._fields_:
        w = rt.RevisionView(*(None if f == name else getattr(v, f) for f, _ in v._fields_))
        assert L.kad_revision_plan_check(ctypes.byref(b), ctypes.byref(w)) == rt.KAD_EINVAL, name


def test_check_unsupported_and_nospc(rt):
    e = HC.sized_obj(H.MAX_REVISIONS)
    ok = HC.batch_of_entries([e]).arrays()
    assert rt.revision_plan_check(**ok) == 0
    # one more revision than the bound (the packing refuses it: extend the arrays of the largest it takes)
    a = dict(ok)
    a["rev_off"] = np.array([0, H.MAX_REVISIONS + 1], np.int32)
    for k in ("rev_data_off", "rev_data_len", "rev_revision", "rev_time", "rev_name_rank", "rev_flags", "rev_hash"):
        a[k] = np.concatenate((a[k], a[k][-1:]))
    a["rev_lab_off"] = np.concatenate((a["rev_lab_off"], a["rev_lab_off"][-1:]))
    assert rt.revision_plan_check(**a) == rt.KAD_EUNSUPPORTED
    with pytest.raises(ValueError):
        HC.batch_of_entries([HC.sized_obj(H.MAX_REVISIONS + 1)])
    g = good()
    R_, O = len(g["rev_flags"]), len(g["obj_flags"])
    assert rt.revision_plan_check(**g, action_capacity=2 * R_ + O) == 0
    assert rt.revision_plan_check(**g, action_capacity=2 * R_ + O - 1) == rt.KAD_ENOSPC


# ------------------------------------------------------------------ kad_revision_plan_route_eval
def test_route_boundaries(rt):
    ev = rt.revision_plan_route_eval
    r = ev(0, 0, 0, 0, 0, 0)
    assert (r["hash_grid"], r["cmp_grid"], r["grid"], r["long_grid"], r["threads"]) == (0, 0, 0, 0, 256)
    assert r["long_min"] == 256 and r["width"] == 1 and r["cmp_width"] == 1
    # the plan kernel's width: the mean revisions of a short object (one a lane), rounded up to a power of two
    for mean, w in [(0, 1), (1, 1), (2, 2), (3, 4), (4, 4), (5, 8), (8, 8), (9, 16), (16, 16), (17, 32), (32, 32), (33, 64), (64, 64), (65, 64), (256, 64)]:
        assert ev(1000, 1000, 0, 1000 * mean, 1000 * mean, 0)["width"] == w, mean
    assert ev(1000, 1000, 0, 2001, 2001, 0)["width"] == 4  # the mean rounds up
    # the compare kernel's width: the mean 16-byte chunks of a pair, four a lane
    for chunks, w in [(0, 1), (4, 1), (5, 2), (8, 2), (9, 4), (16, 4), (17, 8), (128, 32), (129, 64), (256, 64), (257, 64), (100000, 64)]:
        assert ev(10, 10, 0, 100, 100, 100 * chunks)["cmp_width"] == w, chunks
    # grids: a lane per hashed object; 256 / width rows a block, 8 blocks a CU at most
    assert [ev(n, n, 0, 0, 0, 0)["hash_grid"] for n in (1, 256, 257)] == [1, 1, 2]
    assert ev(1000, 10, 0, 1000, 1000, 0)["hash_grid"] == 1
    assert ev(256, 256, 0, 256, 256, 0)["grid"] == 1 and ev(257, 257, 0, 257, 257, 0)["grid"] == 2
    assert ev(10 ** 6, 10 ** 6, 0, 10 ** 6, 10 ** 6, 0, 4)["grid"] == 32
    assert ev(100, 100, 0, 6400, 6400, 0)["grid"] == 25 and ev(100, 100, 0, 6400, 6400, 0)["cmp_grid"] == 25
    # long objects take a block each and leave the group path's mean
    r = ev(10, 10, 3, 7 * 2, 7 * 2 + 3 * 300, 0)
    assert (r["width"], r["grid"], r["long_grid"]) == (2, 1, 3)
    r = ev(3, 3, 3, 0, 900, 0)
    assert (r["grid"], r["long_grid"]) == (0, 3)
    for bad in [(-1, 0, 0, 0, 0, 0), (1, 2, 0, 0, 0, 0), (1, 1, 2, 0, 0, 0), (1, 1, 0, -1, 0, 0), (1, 1, 0, 0, -1, 0), (1, 1, 0, 0, 0, -1)]:
        with pytest.raises(rt.KadError):
            ev(*bad)
    with pytest.raises(rt.KadError):
        ev(1, 1, 0, 0, 0, 0, 0)


def test_reconciler_skips_types_without_revision_history():
    """No device is touched for a type without revisionHistoryEnabled (sync/controller.go:401)."""
    from kubeadmiral_amd import objects as O
    from kubeadmiral_amd.controller import BatchReconciler
    rec = BatchReconciler.__new__(BatchReconciler)
    rec.type_config = O.FederatedTypeConfig("apps", "v1", "Deployment", "deployments")
    out = rec.reconcile_revisions([{"spec": {"revisionHistoryLimit": 3}}], [[]])
    assert [R.outcome_tuple(o) for o in out] == [("AllOK", None, [], None, "", "")]


def test_list_revisions_filter():
    fed = {"metadata": {"name": "web", "namespace": "ns", "uid": "u1"}}
    mk = lambda name, ns="ns", uid="u1", owner=None: {"metadata": {"name": name, "namespace": ns, "labels": {"uid": uid},  # noqa: E731
                                                                     "ownerReferences": owner or []}}
    store = [mk("mine", owner=[{"uid": "u1", "controller": True}]), mk("orphan"), mk("other-ns", ns="x"), mk("other-uid", uid="u2"),
             mk("other-owner", owner=[{"uid": "u9", "controller": True}]), mk("non-controller-ref", owner=[{"uid": "u9"}])]
    assert [r["metadata"]["name"] for r in H.list_revisions(fed, store)] == ["mine", "orphan", "non-controller-ref"]


def test_shared_header_under_sanitizers(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler")
    exe = str(tmp_path / "history_main")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
                    "-static-libasan", "-static-libubsan", os.path.join(HERE, "history_main.cpp"), "-o", exe], check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="halt_on_error=1")
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, env=env, timeout=120)
    out = r.stdout.decode(errors="replace")
    assert r.returncode == 0, out
    assert out.startswith("ok: "), out
