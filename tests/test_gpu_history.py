"""kad_revision_plan on an MI355X == the per-object reference (history_ref.py), exactly: actions, their order and every
string, through Context.revision_plan + RevisionBatch.apply and through BatchReconciler.reconcile_revisions; and its
arrays == history.plan_numpy's.

The hand-written cases and seeded fuzz; objects of 63, 64, 65 and long_min - 1, long_min, long_min + 1 revisions; every
lane-group width and the long path forced through kad_revision_plan_debug_route; patches of lengths around the hash
kernel's tile and its multiples, and one patch 100 times longer than its 63 wave-mates; O = 0 and O = 1. Every device
call runs under a deadline of its own (``within``): a call that does not return ends the session instead of holding it."""
import concurrent.futures

import numpy as np
import pytest

import history_cases as HC
import history_ref as R
from kubeadmiral_amd import history as H
from kubeadmiral_amd import synth

pytestmark = pytest.mark.gpu

WIDTHS = (1, 2, 4, 8, 16, 32, 64)
DEADLINE_S = 60
_POOL = concurrent.futures.ThreadPoolExecutor(max_workers=1)
_NAMED = HC.named()
_ENTRIES = [e for _, (e, _, _) in sorted(_NAMED.items())]
_WANT = [R.sync_revisions(e) for e in _ENTRIES]  # computed once, shared, never changed


def within(fn, *args, **kw):
    """fn(*args) with a deadline: the library call releases the interpreter lock, so a hung device shows here."""
    f = _POOL.submit(fn, *args, **kw)
    try:
        return f.result(timeout=DEADLINE_S)
    except concurrent.futures.TimeoutError:
        pytest.exit(f"a device call did not return within {DEADLINE_S} s", returncode=3)


@pytest.fixture(scope="module")
def ctx():
    from kubeadmiral_amd import build, runtime
    build.build()
    c = within(runtime.Context, 0)
    yield c
    c.close()


def plan(ctx, batch, width=0, long_min=0):
    ctx.revision_plan_debug_route(width, long_min)
    try:
        return within(ctx.revision_plan, **batch.arrays())
    finally:
        ctx.revision_plan_debug_route(0, 0)


def same_arrays(batch, res):
    """The device's arrays against plan_numpy's, wherever they are specified."""
    a = batch.arrays()
    want = H.plan_numpy(**a)
    for k in ("out_off", "hash", "upd_hash", "upd_parsed", "n_old", "keep", "n_actions", "last", "rev_number"):
        assert res[k].tolist() == want[k].tolist(), k
    live = np.repeat(a["limit"] != 0, np.diff(a["rev_off"]))
    assert res["equal"][live].tolist() == want["equal"][live].tolist()
    for o in range(len(a["limit"])):
        lo, n = int(a["rev_off"][o]), int(want["n_old"][o])
        assert res["order"][lo:lo + n].tolist() == want["order"][lo:lo + n].tolist(), o
        lo, n = int(want["out_off"][o]), int(want["n_actions"][o])
        for k in ("act_kind", "act_rev"):
            assert res[k][lo:lo + n].tolist() == want[k][lo:lo + n].tolist(), (o, k)


def check(ctx, entries, want=None, width=0, long_min=0):
    batch = HC.batch_of_entries(entries)
    res = plan(ctx, batch, width, long_min)
    got = [R.outcome_tuple(o) for o in batch.apply(res)]
    assert got == (want if want is not None else [R.sync_revisions(e) for e in entries])
    same_arrays(batch, res)
    return batch, res


def test_named_cases(ctx):
    check(ctx, _ENTRIES, _WANT)
    for e, w in zip(_ENTRIES, _WANT):  # and each alone: O = 1
        check(ctx, [e], [w])


@pytest.mark.parametrize("width", WIDTHS)
def test_named_cases_at_every_forced_width(ctx, width):
    check(ctx, _ENTRIES, _WANT, width)
    r = ctx.revision_plan_last_route()
    assert r["width"] == width and r["cmp_width"] == width


def test_named_cases_on_the_long_path(ctx):
    check(ctx, _ENTRIES, _WANT, long_min=1)
    r = ctx.revision_plan_last_route()
    assert r["long_min"] == 1 and 0 < r["long_grid"] < len(_ENTRIES) and r["grid"] > 0
    check(ctx, _ENTRIES, _WANT, 64, long_min=2)


def test_through_the_reconciler(ctx):
    from kubeadmiral_amd import objects as O
    from kubeadmiral_amd.controller import BatchReconciler
    ftc = O.FederatedTypeConfig("apps", "v1", "Deployment", "deployments", revision_history=True)
    rec = BatchReconciler(ftc, ctx=ctx)

    def fed(name, image, limit, labels=None, collision=None, template=True):
        o = {"metadata": {"name": name, "namespace": "ns", "uid": "uid-" + name, "labels": labels or {}},
             "spec": {"revisionHistoryLimit": limit, "template": {"spec": {"template": {"spec": {"containers": [{"image": image, "cpu": 0.5}]}}}}}}
        if collision is not None:
            o["status"] = {"collisionCount": collision}
        if not template:
            del o["spec"]["template"]["spec"]["template"]
        return o

    feds = [fed("web", "a:2", 2, {"app": "web"}), fed("db", "d:1", 1, collision=3), fed("off", "x", 0), fed("broken", "x", 3, template=False),
            fed("blank", "b:1", 5, {"opt": ""})]
    old_web = H.get_patch(fed("web", "a:1", 2))
    store = [HC.rev("web-1", 1, old_web, {"uid": "uid-web", "app": "web"}, t="2024-01-01T00:00:00Z"),
             HC.rev("web-2", 2, H.get_patch(feds[0]), {"uid": "uid-web"}, t="2024-01-02T00:00:00Z"),
             HC.rev("web-0", 1, old_web.replace(b"a:1", b"a:0"), {"uid": "uid-web", "app": "web"}, t="2024-01-01T00:00:00Z"),
             HC.rev("web-x", 0, old_web.replace(b"a:1", b"a:9"), {"uid": "uid-web", "app": "web"}, t="2023-01-01T00:00:00Z"),
             HC.rev("db-1", 4, H.get_patch(feds[1]), {"uid": "uid-db"}), HC.rev("blank-1", 1, b"[]", {"uid": "uid-blank"}),
             HC.rev("stray", 1, b"[]", {"uid": "uid-other"})]
    for r in store:
        r["metadata"]["namespace"] = "ns"
    listed = [H.list_revisions(f, store) for f in feds]
    assert [len(x) for x in listed] == [4, 1, 0, 0, 1]
    got = within(rec.reconcile_revisions, feds, listed, [None, "77f", None, None, "c4"])
    entries = H.batch_of(feds, listed, [None, "77f", None, None, "c4"]).objs
    for e in entries:  # the reference takes seconds
        for r in e["revisions"]:
            r["metadata"]["creationTimestamp"] = H.seconds(r["metadata"]["creationTimestamp"])
    assert [R.outcome_tuple(o) for o in got] == [R.sync_revisions(e) for e in entries]
    web, db, off, broken, blank = got
    assert web.actions == [("relabel", "web-2", 2), ("delete", "web-x", 0)] and web.last_revision_name_with_hash == "web-1"
    assert db.actions == [] and db.collision_count == 3 and db.current_revision_name.startswith("db-")
    assert (off.actions, off.current_revision_name, off.collision_count) == ([], "", 0)
    assert broken.status == "Error" and "not found" in broken.error
    assert [k for k, _, _ in blank.actions] == ["create"] and blank.last_revision_name_with_hash == "blank-1|c4"


@pytest.mark.parametrize("seed,width", [(11, 0), (12, 2), (13, 64)])
def test_fuzz(ctx, seed, width):
    entries = HC.random_objs(seed, 400)
    batch, res = check(ctx, entries, width=width)
    a = batch.arrays()
    hosted = (a["obj_flags"] & H.OBJ_LABELS_ON_HOST) != 0
    assert 0 < int(hosted.sum()) < len(entries) // 4
    for o in np.nonzero(hosted)[0]:  # the device emits no relabel for an object whose label tests are the host's
        lo = int(res["out_off"][o])
        assert 4 not in res["act_kind"][lo:lo + int(res["n_actions"][o])].tolist()


def test_gen_revisions(ctx):
    batch = synth.gen_revisions(3, 300, long_every=64)
    res = plan(ctx, batch)
    assert [R.outcome_tuple(o) for o in batch.apply(res)] == [R.sync_revisions(e) for e in batch.objs]
    same_arrays(batch, res)
    assert ctx.revision_plan_last_route()["hash_grid"] == 2


def test_revisions_around_the_group_and_the_long_path(ctx):
    from kubeadmiral_amd import runtime
    long_min = runtime.revision_plan_route_eval(0, 0, 0, 0, 0, 0)["long_min"]
    sizes = [63, 64, 65, long_min - 1, long_min, long_min + 1]
    entries = [HC.sized_obj(n, seed=n, limit=n // 3) for n in sizes]
    want = [R.sync_revisions(e) for e in entries]
    assert all(len(w[2]) > n // 2 for w, n in zip(want, sizes))
    check(ctx, entries, want)
    r = ctx.revision_plan_last_route()
    assert r["long_grid"] == 1 and r["width"] == 64
    check(ctx, entries, want, long_min=63)  # all but the first a block each
    assert ctx.revision_plan_last_route()["long_grid"] == 5
    check(ctx, entries, want, 64, long_min=1 << 20)  # all on 64-lane groups: five passes over 257
    assert ctx.revision_plan_last_route()["long_grid"] == 0
    check(ctx, entries, want, 1, long_min=1 << 20)


def test_hash_lengths_around_the_tile(ctx):
    lens = [0, 1, 3, 4, 5, 15, 16, 17, 63, 64, 65, 127, 128, 129, 191, 192, 193, 255, 256, 257, 4095, 4096, 4097]
    entries = [HC.obj([], patch=HC.pattern(n, salt=n), collision=c, name=f"p{n}") for n in lens for c in (None, 7)]
    batch, res = check(ctx, entries)
    for e, h in zip(entries, res["hash"].tolist()):
        want = R.fnv1_32(e["patch"])
        if e["collision"] is not None:
            want = R.fnv1_32(b"7", want)
        assert h == want, len(e["patch"])


def test_one_patch_100_times_longer_than_its_wave_mates(ctx):
    entries = [HC.obj([HC.rev("r", 1, HC.pattern(64, salt=i))], patch=HC.pattern(6400 if i == 37 else 64, salt=i), collision=None, name=f"w{i}") for i in range(64)]
    batch, res = check(ctx, entries)
    assert res["hash"].tolist() == [R.fnv1_32(e["patch"]) for e in entries]
    assert res["equal"].tolist() == [0 if i == 37 else 1 for i in range(64)]
    # and 300 objects, the long one in the second wave of the second block's order
    more = [HC.obj([], patch=HC.pattern(6400 if i == 150 else 40 + i % 50, salt=i), collision=None, name=f"m{i}") for i in range(300)]
    batch, res = check(ctx, more)
    assert res["hash"].tolist() == [R.fnv1_32(e["patch"]) for e in more]


def test_empty_and_single(ctx):
    from kubeadmiral_amd import runtime
    one = [_NAMED["old_ties_by_time_then_name"][0]]
    check(ctx, one)
    route = ctx.revision_plan_last_route()
    assert (route["hash_grid"], route["cmp_grid"], route["grid"]) == (1, 1, 1)
    ms = ctx.revision_plan_timing()
    assert len(ms) == 3 and all(np.isfinite(m) and m >= 0 for m in ms)
    none = plan(ctx, HC.batch_of_entries([]))
    assert len(none["hash"]) == 0 and none["out_off"].tolist() == [0] and ctx.revision_plan_last_route() == route
    first, again = plan(ctx, HC.batch_of_entries(one)), plan(ctx, HC.batch_of_entries(one))
    assert all(first[k].tobytes() == again[k].tobytes() for k in ("hash", "equal", "n_actions", "keep", "last"))
    bad = HC.batch_of_entries(one).arrays()
    bad["rev_name_rank"] = np.full_like(bad["rev_name_rank"], 9)
    with pytest.raises(runtime.KadError) as e:
        within(ctx.revision_plan, **bad)
    assert e.value.code == runtime.KAD_EINVAL and ctx.revision_plan_last_route() == route
    limits_only = [HC.obj([HC.rev("r", 1, HC.P)], limit=0, name=f"z{i}") for i in range(3)]
    check(ctx, limits_only)  # nothing to hash: the hash kernel is not launched
    assert ctx.revision_plan_last_route()["hash_grid"] == 0
