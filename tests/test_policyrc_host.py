"""kad_policyrc_count without a GPU: the library's validation and launch decision, and PolicyRefCounter's packing
and status writes (arrays → the numpy checker → apply) against the per-event checker (policyrc_ref.py) on seeded
event streams and on the scenario of the reference's counter_test.go."""
import numpy as np
import pytest

import policyrc_cases as PC
import policyrc_ref as R
from kubeadmiral_amd import policyrc as PR


@pytest.fixture(scope="module")
def runtime():
    from kubeadmiral_amd import build, runtime
    build.build()
    return runtime


def test_constants_agree():
    assert (PR.POL_EXISTS, PR.POL_ENQUEUED, PR.FLAGGED, PR.UPDATE, PR.NEGATIVE) == \
        (R.POL_EXISTS, R.POL_ENQUEUED, R.FLAGGED, R.UPDATE, R.NEGATIVE) == (1, 2, 1, 2, 4)


def test_validation(runtime):
    arr, _ = PC.case("random", 33, 100, 90, 1)
    arr = {k: np.array(v) for k, v in arr.items()}
    assert runtime.policyrc_check(**arr) == 0
    assert runtime.policyrc_check(**PC.batch(5, [], [], flags=3)) == 0          # both lists empty (null)
    assert runtime.policyrc_check(**PC.batch(0, [], [])) == 0                   # no policies
    bad = [
        dict(n_policies=-1), dict(n_dec=-1), dict(n_inc=-1),                    # a negative count
        dict(dec_ids=np.zeros(0, np.int32), n_dec=3), dict(inc_ids=np.zeros(0, np.int32), n_inc=1),  # null, count != 0
        dict(count=np.zeros(0, np.int64)), dict(stored_typed=np.zeros(0, np.int64)),
        dict(stored_rest=np.zeros(0, np.int64)), dict(stored_total=np.zeros(0, np.int64)),
        dict(pol_flags=np.zeros(0, np.uint8), n_policies=33),
        dict(dec_ids=np.array([0, 33, 1], np.int32)), dict(dec_ids=np.array([-1], np.int32)),  # an id outside [0, P)
        dict(inc_ids=np.array([5, 4, 33], np.int32)), dict(inc_ids=np.array([-(2 ** 31)], np.int32)),
        dict(pol_flags=np.where(np.arange(33) == 32, 4, arr["pol_flags"]).astype(np.uint8)),    # an unknown flag
        dict(reserved=1),
    ]
    for change in bad:
        assert runtime.policyrc_check(**{**arr, **change}) == runtime.KAD_EINVAL, change
    # a missing output
    b, v, _keep, _out = runtime.policyrc_args(**arr)
    v.state = None
    assert runtime._check("policyrc", (b, v)) == runtime.KAD_EINVAL
    # with no policies every id is outside the table
    assert runtime.policyrc_check(**{**PC.batch(0, [], []), "inc_ids": np.zeros(1, np.int32)}) == runtime.KAD_EINVAL


def test_route(runtime):
    bins = runtime.policyrc_route_eval(1, 1)["bins"]
    assert bins >= 64
    for P, path in ((bins - 1, 0), (bins, 0), (bins + 1, 1)):
        r = runtime.policyrc_route_eval(P, 1 << 20)
        assert r["path"] == path and r["bins"] == bins and r["threads"] == 256 and r["vec"] == 4
        assert r["apply_grid"] == (P + 255) // 256 and r["grid"] >= 1
        # resident blocks bound the grid: a block's 2 * P bins within a CU's 160 KiB on the LDS-private path
        per_cu = min(8, (160 * 1024) // (8 * P)) if path == 0 else 8
        assert r["grid"] == min(1 << 10, 256 * per_cu)
    none = runtime.policyrc_route_eval(1000, 0)
    assert none["grid"] == 0 and none["apply_grid"] == 4 and none["path"] == 0
    assert runtime.policyrc_route_eval(1000, 1)["grid"] == 1 and runtime.policyrc_route_eval(1000, 1025)["grid"] == 2
    assert runtime.policyrc_route_eval(bins, 1 << 24, 4)["grid"] == 4 * min(8, (160 * 1024) // (8 * bins))
    for args in ((-1, 0, 256), (1, -1, 256), (1, 1, 0)):
        with pytest.raises(runtime.KadError) as e:
            runtime.policyrc_route_eval(*args)
        assert e.value.code == runtime.KAD_EINVAL


@pytest.mark.parametrize("namespaced", [True, False])
def test_counter_equals_the_reference_on_a_stream(namespaced):
    batches = PC.stream(namespaced, 11)
    counter, ctrl, n_updates = PC.walk(namespaced, batches, PC.policy_store(namespaced, 3), PC.via_numpy)
    assert n_updates > 10
    events = [e for b, _ in batches for e in b]
    assert any(obj is None for _, obj in events)
    names = [n for n, _ in batches[0][0]]
    assert len(names) > len(set(names))                                        # one object several times in a batch
    assert any(k[2] == "p5" for k in counter.keys) == namespaced               # a policy the store lacks
    assert ("override", "", "co1") in counter.ids
    if not namespaced:  # the override-policy label on a cluster-scoped object counts, with an empty namespace
        assert any(k[0] == "override" and k[1] == "" and k[2].startswith("o") for k in counter.keys)
        assert not any(k[2].startswith("p") for k in counter.keys)


def test_enqueued_untouched_policy_is_persisted():
    """A stale stored count on a policy that no event names: written only when the policy is enqueued."""
    key = ("propagation", "ns0", "p0")
    store = {key: {"metadata": {"name": "p0", "namespace": "ns0"},
                   "status": {"refCount": 9, "typedRefCount": [{"group": PC.GROUP, "resource": PC.RESOURCE, "count": 9}]}}}
    counter = PR.PolicyRefCounter(PC.ftc())
    other = PC.fed_object("ns0", "a", pp="p1")
    assert PC.via_numpy(counter, [("ns0/a", other)], store, []) == ([("propagation", "ns0", "p1")], [])
    flagged, updates = PC.via_numpy(counter, [], store, [key])
    assert flagged == [] and updates == [(key, store[key])]
    assert store[key]["status"] == {"refCount": 0, "typedRefCount": [{"group": PC.GROUP, "resource": PC.RESOURCE, "count": 0}]}


def test_pass_through_policy_is_flagged():
    """a → b → a within one batch: b's count does not move, the reference flags it all the same."""
    counter = PR.PolicyRefCounter(PC.ftc())
    obj = lambda p: PC.fed_object("ns0", "x", pp=p)  # noqa: E731
    PC.via_numpy(counter, [("ns0/x", obj("a"))], {}, [])
    counter.observe([("ns0/x", obj("b")), ("ns0/x", obj("a"))])
    arrays = counter.arrays({}, [])
    assert arrays["dec_ids"].tolist() == arrays["inc_ids"].tolist() == [counter.ids[("propagation", "ns0", "a")]]
    flagged, _ = counter.apply(R.run(**arrays), {})
    assert set(flagged) == {("propagation", "ns0", "a"), ("propagation", "ns0", "b")}
    assert counter.get_policy_counts([("propagation", "ns0", "a"), ("propagation", "ns0", "b")]) == [1, 0]


def test_negative_count_raises_with_the_reference_message():
    counter = PR.PolicyRefCounter(PC.ftc())
    key = ("propagation", "ns0", "a")
    PC.via_numpy(counter, [("ns0/x", PC.fed_object("ns0", "x", pp="a"))], {}, [])
    counter.counts[counter.ids[key]] = 0  # bookkeeping gone wrong
    ref = R.Counter()
    ref.known["ns0/x"] = [("ns0", "a")]
    with pytest.raises(RuntimeError) as want:
        ref.update("ns0/x", [])
    with pytest.raises(PR.PolicyRefCountError) as got:
        PC.via_numpy(counter, [("ns0/x", None)], {}, [])
    assert str(got.value) == str(want.value) == "counter.policyCounts[{ns0 a}] must be non-negative"


def test_golden_scenario():
    g, batches = PC.golden_batches()
    assert sum(len(b) for b in batches) == 4096 and len(batches) == 8
    counter, ctrl, _ = PC.walk(False, [(b, []) for b in batches], {}, PC.via_numpy)
    keys = [("propagation", "", str(p)) for p in range(g["num_policies"])]
    assert set(keys) == {("propagation",) + k for k in ctrl.pp.flagged} and len(keys) == g["expect_flagged_policies"]
    assert sum(counter.get_policy_counts(keys)) == g["expect_count_sum"] == sum(ctrl.pp.get_policy_counts([k[1:] for k in keys]))
