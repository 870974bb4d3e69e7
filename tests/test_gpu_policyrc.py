"""kad_policyrc_count on an MI355X == the numpy checker (policyrc_ref.run), exactly: every output is an integer.

P of 1, 2, 31/32/33, 63/64/65 and bins - 1 / bins / bins + 1 (the bins limit read from the route), the small ones on
both paths; id lists of 0, 1, 3, 4, 5, 255, 256, 257 ids and of one grid step of the LDS-private route - 1 / + 0 / + 1
(at P = bins the step is grid x 256 x 4 = 2 blocks a CU; the global path's step, 8 blocks a CU, is above the 1M ids
a test list may hold, so its second stride is not reached here); every id on one policy; runs of 1, 63, 64, 65 and
200 equal ids; random ids; a policy removed and added equally often; int64 wrap; a negative count; the staging buffer
growing, reused and shrinking; a kad_group member; reconcile_policy_refcounts end to end against the per-event
checker."""
import numpy as np
import pytest

import policyrc_cases as PC
import policyrc_ref as R

pytestmark = pytest.mark.gpu

OWN, LDS, GLOBAL = 0, 1, 2


@pytest.fixture(scope="module")
def ctx():
    from kubeadmiral_amd import build, runtime
    build.build()
    c = runtime.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def bins():
    from kubeadmiral_amd import runtime
    return runtime.policyrc_route_eval(1, 1)["bins"]


def count(ctx, arr, force=OWN):
    ctx.policyrc_debug_route(force)
    try:
        return ctx.policyrc_count(**arr)
    finally:
        ctx.policyrc_debug_route(OWN)


def check(ctx, key, force=OWN, path=None):
    arr, want = PC.case(*key)
    got = count(ctx, arr, force)
    assert PC.equal(got, want) is None, (key, force)
    route = ctx.policyrc_last_route()
    if path is not None:
        assert route["path"] == path
    return route


@pytest.mark.parametrize("force", [OWN, GLOBAL])
@pytest.mark.parametrize("P", [1, 2, 31, 32, 33, 63, 64, 65])
def test_small_tables_on_both_paths(ctx, P, force):
    route = check(ctx, ("random", P, 1000, 900, P), force, path=1 if force == GLOBAL else 0)
    assert route["grid"] == 2 and route["apply_grid"] == 1


@pytest.mark.parametrize("d", [-1, 0, 1])
def test_bins_boundary(ctx, bins, d):
    P = bins + d
    route = check(ctx, ("random", P, 50000, 40000, 5), path=1 if d > 0 else 0)
    assert route["bins"] == bins and route["apply_grid"] == (P + 255) // 256
    if d <= 0:  # and the same table through the global path
        check(ctx, ("random", P, 50000, 40000, 5), GLOBAL, path=1)
    else:
        from kubeadmiral_amd import runtime
        arr, _ = PC.case("random", P, 50000, 40000, 5)
        with pytest.raises(runtime.KadError) as e:
            count(ctx, arr, LDS)
        assert e.value.code == runtime.KAD_EINVAL


@pytest.mark.parametrize("force", [OWN, GLOBAL])
def test_empty_lists(ctx, force):
    """No ids in either list or in both: the count kernel has nothing to do (grid 0 with both empty), the apply
    kernel still persists the enqueued policies."""
    ids = PC.random_ids(4, 700, 40)
    for dec, inc in ((ids, []), ([], ids), ([], [])):
        arr = PC.batch(40, dec, inc, 9, flags=R.POL_EXISTS | R.POL_ENQUEUED)
        want = R.run(**arr)
        got = count(ctx, arr, force)
        assert PC.equal(got, want) is None
        assert (got["state"] & R.UPDATE).any() and ((got["state"] & R.FLAGGED) != 0).any() == bool(len(dec) + len(inc))
        assert ctx.policyrc_last_route()["grid"] == (1 if len(dec) + len(inc) else 0)


@pytest.mark.parametrize("force", [OWN, GLOBAL])
@pytest.mark.parametrize("n", [1, 3, 4, 5, 255, 256, 257])
def test_list_lengths(ctx, n, force):
    check(ctx, ("random", 97, n, 0, n), force)
    check(ctx, ("random", 97, 7, n, n), force)
    check(ctx, ("random", 97, n, n, n), force)


def test_one_grid_step(ctx, bins):
    """Lists of one grid step of the LDS-private route at P = bins, one id less and one more: with one more, block 0
    takes a second step of the list."""
    route = check(ctx, ("random", bins, 600000, 600000, 3), path=0)
    step = route["grid"] * route["threads"] * route["vec"]
    assert route["grid"] >= 2 and step + 1 <= 1 << 20 and 1200000 >= step
    for nd, ni in ((step - 1, step + 1), (step, step - 1), (step + 1, step)):
        r = check(ctx, ("random", bins, nd, ni, 8), path=0)
        assert r["grid"] == route["grid"]


@pytest.mark.parametrize("force,P", [(OWN, 1000), (GLOBAL, 1000), (OWN, 20000)])
def test_every_id_on_one_policy(ctx, P, force):
    arr, want = PC.case("one", P, 100000)
    got = count(ctx, arr, force)
    assert PC.equal(got, want) is None
    assert np.flatnonzero(got["state"] & R.FLAGGED).tolist() == [P // 2]


@pytest.mark.parametrize("force,P", [(OWN, 97), (GLOBAL, 97), (OWN, 20000)])
@pytest.mark.parametrize("run", [1, 63, 64, 65, 200])
def test_runs_of_equal_ids(ctx, run, P, force):
    """Runs that end inside a lane's four ids, at a lane's edge, at a wave's 256 ids and across blocks."""
    check(ctx, ("runs", P, 5000, run), force)
    check(ctx, ("runs", P, 2 * 1024 + 3, run), force)


@pytest.mark.parametrize("force,P", [(OWN, 1000), (GLOBAL, 1000), (OWN, 100000)])
def test_random_ids(ctx, P, force):
    route = check(ctx, ("random", P, 200000, 150000, 21), force)
    assert route["grid"] == (350000 + 1023) // 1024


@pytest.mark.parametrize("force", [OWN, GLOBAL])
def test_removed_and_added_equally_often(ctx, force):
    i64 = lambda *v: np.array(v, np.int64)  # noqa: E731
    arr = {"dec_ids": np.array([1, 1], np.int32), "inc_ids": np.array([1, 1], np.int32), "count": i64(0, 2, 0),
           "stored_typed": i64(0, 2, 0), "stored_rest": i64(0, 5, 0), "stored_total": i64(0, 7, 0),
           "pol_flags": np.full(3, R.POL_EXISTS, np.uint8)}
    got = count(ctx, arr, force)
    assert PC.equal(got, R.run(**arr)) is None
    assert got["state"].tolist() == [0, R.FLAGGED, 0] and got["new_count"].tolist() == [0, 2, 0]
    arr["stored_total"] = i64(0, 8, 0)  # the stored sum is stale: now it is an update
    assert count(ctx, arr, force)["state"].tolist() == [0, R.FLAGGED | R.UPDATE, 0]


def test_int64_wrap(ctx):
    i64 = lambda *v: np.array(v, np.int64)  # noqa: E731
    arr = {"dec_ids": np.array([1], np.int32), "inc_ids": np.array([0, 0, 1], np.int32), "count": i64(2 ** 62, 2 ** 63 - 1),
           "stored_typed": i64(0, 0), "stored_rest": i64(2 ** 63 - 1, -(2 ** 63)), "stored_total": i64(0, -1),
           "pol_flags": np.full(2, R.POL_EXISTS, np.uint8)}
    got = count(ctx, arr)
    assert PC.equal(got, R.run(**arr)) is None
    assert got["new_count"].tolist() == [2 ** 62 + 2, 2 ** 63 - 1]
    assert got["new_total"].tolist() == [R.wrap(2 ** 63 - 1 + 2 ** 62 + 2), -1]
    assert got["state"].tolist() == [R.FLAGGED | R.UPDATE, R.FLAGGED | R.UPDATE]


def test_negative_count(ctx):
    arr = PC.batch(9, [], [], 1)
    arr["count"] = np.zeros(9, np.int64)
    arr["dec_ids"] = np.array([4], np.int32)
    got = count(ctx, arr)
    assert PC.equal(got, R.run(**arr)) is None
    assert got["n_negative"].tolist() == [1] and got["new_count"][4] == -1
    assert [bool(s & R.NEGATIVE) for s in got["state"]] == [i == 4 for i in range(9)]
    # and the Python layer raises where the reference panics
    from kubeadmiral_amd import policyrc as PR
    from kubeadmiral_amd.controller import BatchReconciler
    rec = BatchReconciler(PC.ftc(), ctx=ctx)
    rec.reconcile_policy_refcounts([("ns0/x", PC.fed_object("ns0", "x", pp="a"))], {})
    rec.policy_refs.counts[0] = 0
    with pytest.raises(PR.PolicyRefCountError) as e:
        rec.reconcile_policy_refcounts([("ns0/x", None)], {})
    assert str(e.value) == "counter.policyCounts[{ns0 a}] must be non-negative"


def test_staging_buffer_grows_is_reused_and_shrinks():
    from kubeadmiral_amd import runtime
    c = runtime.Context(0)
    try:
        for f in (c.policyrc_timing, c.policyrc_last_route):
            with pytest.raises(runtime.KadError) as e:
                f()
            assert e.value.code == runtime.KAD_ESTATE
        tiny, want = PC.case("random", 33, 100, 90, 1)
        first = c.policyrc_count(**tiny)
        assert PC.equal(first, want) is None
        ms = c.policyrc_timing()
        assert len(ms) == 3 and all(np.isfinite(m) and m >= 0 for m in ms)
        big, big_want = PC.case("random", 100000, 200000, 150000, 21)
        assert PC.equal(c.policyrc_count(**big), big_want) is None
        again = c.policyrc_count(**tiny)
        for k in first:
            assert np.asarray(again[k]).tobytes() == np.asarray(first[k]).tobytes(), k
        # no policies: nothing launches, the last route stays
        route = c.policyrc_last_route()
        none = c.policyrc_count(**PC.batch(0, [], []))
        assert all(len(none[k]) == 0 for k in ("new_count", "new_total", "state")) and none["n_negative"].tolist() == [0]
        assert c.policyrc_last_route() == route
        with pytest.raises(runtime.KadError) as e:
            c.policyrc_count(**{**tiny, "inc_ids": np.array([33], np.int32)})
        assert e.value.code == runtime.KAD_EINVAL and c.policyrc_last_route() == route
    finally:
        c.close()


def test_group_member(ctx):
    from kubeadmiral_amd import runtime
    arr, want = PC.case("random", 65, 1000, 900, 65)
    g = runtime.GroupContext([0, 0])
    try:
        assert PC.equal(g.member(1).policyrc_count(**arr), want) is None
    finally:
        g.close()


def reconciler(ctx, namespaced):
    """A BatchReconciler, its counter, and the call that takes one batch through reconcile_policy_refcounts."""
    from kubeadmiral_amd import policyrc as PR
    from kubeadmiral_amd.controller import BatchReconciler
    rec = BatchReconciler(PC.ftc(namespaced), ctx=ctx)
    rec.policy_refs = PR.PolicyRefCounter(rec.type_config)
    return rec, lambda counter, events, store, enqueued: rec.reconcile_policy_refcounts(events, store, enqueued)


@pytest.mark.parametrize("namespaced", [True, False])
def test_reconcile_policy_refcounts_on_a_stream(ctx, namespaced):
    rec, via = reconciler(ctx, namespaced)
    _, _, n_updates = PC.walk(namespaced, PC.stream(namespaced, 11), PC.policy_store(namespaced, 3), via, rec.policy_refs)
    assert n_updates > 10 and ctx.policyrc_last_route()["path"] == 0


def test_reconcile_policy_refcounts_on_the_golden_scenario(ctx):
    g, batches = PC.golden_batches()
    rec, via = reconciler(ctx, False)
    PC.walk(False, [(b, []) for b in batches], {}, via, rec.policy_refs)
    keys = [("propagation", "", str(p)) for p in range(g["num_policies"])]
    assert sorted(rec.policy_refs.keys) == sorted(keys) and len(keys) == g["expect_flagged_policies"]
    assert sum(rec.policy_refs.get_policy_counts(keys)) == g["expect_count_sum"]
