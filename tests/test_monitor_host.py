"""The monitor's host half without a GPU: kubeadmiral_amd.monitor's packing and numpy restatements against the
per-object checker (monitor_ref.py) on the named and seeded cases, the RFC3339Nano parser, slot reuse, duplicate keys,
the metrics' names and tags, the golden file, and the library's host-only entry points (check, route_eval)."""
import json

import numpy as np
import pytest

import monitor_cases as MC
import monitor_ref as R
from kubeadmiral_amd import monitor as M
from kubeadmiral_amd import runtime

T0, S, MIN = MC.T0, MC.S, MC.MIN


@pytest.mark.parametrize("name", sorted(MC.CASES))
def test_named_case(name):
    assert MC.run_case(MC.CASES[name], MC.NumpyBackend) is None


@pytest.mark.parametrize("seed", range(6))
def test_seeded(seed):
    assert MC.run_seeded(seed, MC.NumpyBackend) is None


def test_golden_file_is_the_checkers():
    with open(MC.GOLDEN) as f:
        assert json.load(f) == json.loads(json.dumps(MC.golden()))


def test_branches_are_reached():
    """The named cases reach every result and every bit."""
    results, flags = set(), set()
    for case in MC.CASES.values():
        h = MC.Harness(MC.NumpyBackend)
        h.seed(case.get("seed", ()))
        for now, e in case["steps"]:
            o = h.table.reconcile([e], now, h.be.run, h.be.reserve)[0]
            results.add(o.result)
            flags |= {k for k in ("update_annotation", "meter_deleted", "status_stored", "missing_observed_generation") if getattr(o, k)}
    assert results == {"ALL_OK", "ERROR", "REQUEUE"} and len(flags) == 4


@pytest.mark.parametrize("text,want", [
    ("2023-11-14T22:13:20Z", T0),
    ("2023-11-14T22:13:20.000000001Z", T0 + 1),
    ("2023-11-14T22:13:20.123456789Z", T0 + 123456789),
    ("2023-11-14T22:13:20.5Z", T0 + 500000000),
    ("2023-11-14T22:13:20.1234567891234Z", T0 + 123456789),
    ("2023-11-15T06:13:20+08:00", T0),
    ("2023-11-14T17:43:20.25-04:30", T0 + 250000000),
    ("1970-01-01T00:00:00Z", 0),
    ("0001-01-01T00:00:00Z", -62135596800 * S),
    ("2024-02-29T00:00:00Z", 1709164800 * S),
    ("2023-02-29T00:00:00Z", None), ("2023-11-14 22:13:20Z", None), ("2023-11-14T22:13:20", None),
    ("2023-11-14T24:00:00Z", None), ("2023-11-14T22:13:60Z", None), ("2023-11-14T22:13:20.Z", None),
    ("2023-11-14T22:13:20+0800", None), ("2023-11-14T22:13:20Zjunk", None), ("", None), ("soon", None), (None, None),
    ("２０２３-11-14T22:13:20Z", None),
])
def test_rfc3339nano(text, want):
    assert M.parse_rfc3339nano(text) == want
    ref = R.parse_time(text)
    assert (None if ref is None else ref - R.EPOCH) == want


def test_device_time_range():
    assert M.device_time(None) == M.TIME_ZERO == M.device_time(-62135596800 * S)
    assert M.device_time(T0) == T0
    for bad in (-1, 1 << 62):
        with pytest.raises(ValueError):
            M.device_time(bad)


def test_sat_sub_matches_go():
    """The declared representation against Go's time: every pair of a real time, the zero time and zero - 10 ms."""
    go = [R.unix(T0), R.unix(0), 0, -10 * R.MS, 60 * S]
    for a in go:
        for b in go:
            assert M.sat_sub(MC.dev_time(a), MC.dev_time(b)) == R.go_sub(a, b)
            assert (MC.dev_time(a) > MC.dev_time(b)) == (a > b)


def test_slot_reuse_after_delete():
    t = M.MeterTable()
    be = MC.NumpyBackend(t)
    evs = [MC.ev(MC.synced_obj(), key=f"FederatedDeployment/d/o{i}") for i in range(4)]
    t.reconcile(evs, T0, be.run, be.reserve)
    assert [t.slot_of[e["key"]] for e in evs] == [0, 1, 2, 3]
    t.reconcile([MC.ev(None, key=evs[2]["key"]), MC.ev(None, key=evs[0]["key"])], T0 + S, be.run, be.reserve)
    assert t.capacity_needed == 4 and (be.mirror.flags[:4] == [0, 1, 0, 1]).all()
    t.reconcile([MC.ev(MC.synced_obj(), key="FederatedJob/d/x"), MC.ev(MC.synced_obj(), key="FederatedJob/d/y"),
                 MC.ev(MC.synced_obj(), key="FederatedJob/d/z")], T0 + 2 * S, be.run, be.reserve)
    assert [t.slot_of[f"FederatedJob/d/{k}"] for k in "xyz"] == [0, 2, 4]
    assert be.mirror.type_id[[0, 2, 4]].tolist() == [1, 1, 1] and 0 not in t.last
    assert not hasattr(t, "mirror")  # the table keeps no host copy of the meters


def test_duplicate_keys_split_across_calls():
    evs = [MC.ev(MC.synced_obj(), MC.fed(MC.A2), MC.mem(MC.A2)), MC.ev(MC.synced_obj(), key="FederatedJob/d/b"),
           MC.ev(MC.synced_obj(), MC.fed(MC.A2), MC.mem(MC.A3)), MC.ev(None), MC.ev(MC.synced_obj(), MC.fed(MC.A2), MC.mem(MC.A2))]
    assert M.MeterTable.split(evs) == [[0, 1], [2], [3], [4]]
    with pytest.raises(ValueError):
        M.MonitorBatch.pack(M.MeterTable(), evs, T0)
    h = MC.Harness(MC.NumpyBackend)
    assert h.step(T0, evs) is None
    assert h.table.reconcile(evs[:1], T0, h.be.run)[0].log_last_status == dict(MC.A2)


def test_failed_call_rolls_its_slots_back():
    """A call that raises leaves no key with a slot the device never made live: the key is new again."""
    t = M.MeterTable()
    be = MC.NumpyBackend(t)
    t.reconcile([MC.ev(MC.synced_obj(), key="FederatedJob/d/a")], T0, be.run, be.reserve)

    def broken(*p, **a):
        raise RuntimeError("KAD_EHIP")

    evs = [MC.ev(MC.synced_obj(), key="FederatedJob/d/b"), MC.ev(MC.synced_obj(), key="FederatedJob/d/a"),
           MC.ev(MC.synced_obj(), key="FederatedJob/d/c")]
    with pytest.raises(RuntimeError):
        t.reconcile(evs, T0 + S, broken, be.reserve)
    assert sorted(t.slot_of) == ["FederatedJob/d/a"] and t.key_of == {0: "FederatedJob/d/a"}
    with pytest.raises(RuntimeError):  # a failing reserve too
        t.reconcile(evs, T0 + S, be.run, broken)
    assert sorted(t.slot_of) == ["FederatedJob/d/a"]
    out = t.reconcile(evs, T0 + S, be.run, be.reserve)
    assert [o.result for o in out] == ["ALL_OK"] * 3 and sorted(t.slot_of.values()) == [0, 1, 2]
    assert (be.mirror.flags[:3] == 1).all()


def test_last_status_store_is_a_csr_pool():
    """Lists are appended to one pool, nil is not empty, and the pool is compacted once most of it is garbage."""
    st = M.LastStore()
    rng = np.random.default_rng(0)
    want = {}
    for step in range(4000):
        slot = int(rng.integers(0, 50))
        if rng.random() < 0.1:
            st.pop(slot)
            want.pop(slot, None)
        else:
            n = int(rng.integers(0, 6))
            ids, gens = np.sort(rng.choice(100, n, replace=False)).astype(np.int32), rng.integers(0, 9, n)
            st[slot] = (ids, gens)
            want[slot] = (ids.tolist(), gens.tolist())
    assert {s: (st[s][0].tolist(), st[s][1].tolist()) for s in range(60) if s in st} == want
    assert st.get(55) is None and st.used < 3000 and st.used - st.garbage == sum(len(v[0]) for v in want.values())
    st[7] = ([], [])
    assert 7 in st and st[7][0].tolist() == []
    st.pop(7)
    assert 7 not in st


def test_panics_raise():
    st = dict(metadata={}, clusterStatus=[dict(clusterName="a", status=dict(observedGeneration=1.5))])
    with pytest.raises(TypeError):
        M.MonitorBatch.pack(M.MeterTable(), [MC.ev(MC.synced_obj(), st, MC.mem(MC.A2))], T0)
    with pytest.raises(R.Panic):
        R.Monitor().reconcile(MC.ev(MC.synced_obj(), st, MC.mem(MC.A2)), R.unix(T0))


def test_to_metrics_names_and_tags():
    h = MC.Harness(MC.NumpyBackend)
    h.seed(MC.CASES["late_sync_buckets"]["seed"] + [MC.seed(dict(MC.A2), T0 - 400 * S, 7 * MIN, creation=T0 - 600 * S,
                                                           lu=T0 - 500 * S, ss=T0 - 550 * S, key="FederatedJob/default/late")])
    h.step(T0, [MC.ev(MC.obj(sync=T0 - 5 * S), key="FederatedDeployment/default/fresh")])
    m = M.Report.from_result(h.table, h.be.report(T0, h.table.n_types)).to_metrics()
    names = [x[1] for x in m]
    bucket = ["latency5min", "latency10min", "latency30min", "latency1hour", "latency6hour", "latency1day"]
    assert names[:12] == [b + ".count" for b in bucket] + [b + ".status.count" for b in bucket]
    assert names[-1] == "totalstatus.throughput" and "totalsync.throughput" in names
    by = {(x[1], x[3]): x[2] for x in m}
    assert by[("typelatency5min.count", (("type", "FederatedJob"),))] == 2
    assert by[("typelatency5min.count", (("type", "FederatedDeployment"),))] == 1
    assert by[("typelatency5min.status.count", (("type", "FederatedJob"),))] == 1
    assert ("typelatency5min.status.count", (("type", "FederatedDeployment"),)) not in by  # zero counts are omitted
    assert by[("totalsync.latency.ms", (("resourcename", "FederatedDeployment/default/fresh"),))] == 3595000
    assert by[("totalstatus.latency.ms", (("resourcename", "FederatedJob/default/late"),))] == 420000
    assert by[("latency6hour.count", ())] == 1 and by[("latency1day.count", ())] == 1  # 180 minutes, not 360
    assert sorted(m) == h.ref.metrics(R.unix(T0))


def test_saturated_latency():
    """No creationTimestamp: syncSuccess - zero saturates, Milliseconds() is 9223372036854."""
    h = MC.Harness(MC.NumpyBackend)
    assert h.step(T0, [MC.CASES["no_creation_timestamp"]["steps"][0][1]]) is None
    r = h.be.report(T0, 1)
    assert r["sync_ms"].tolist() == [9223372036854] and h.report_diff(T0) is None


def arrays_of(events, now=T0):
    return M.MonitorBatch.pack(M.MeterTable(), events, now).arrays()


def test_library_check():
    from kubeadmiral_amd import build
    build.build()
    a = arrays_of([MC.ev(MC.synced_obj(), MC.fed(MC.A2), MC.mem(MC.A3)), MC.ev(MC.synced_obj(), key="FederatedJob/d/b")])
    assert runtime.monitor_reconcile_check(**a) == 0
    bad = dict(a, now_ns=-1)
    assert runtime.monitor_reconcile_check(**bad) == runtime.KAD_EINVAL
    bad = dict(a, obj_flags=a["obj_flags"] | 4096)
    assert runtime.monitor_reconcile_check(**bad) == runtime.KAD_EINVAL
    bad = dict(a, mem_cluster=a["mem_cluster"][::-1].copy())
    assert runtime.monitor_reconcile_check(**bad) == runtime.KAD_EINVAL
    bad = dict(a, n_clusters=1)
    assert runtime.monitor_reconcile_check(**bad) == runtime.KAD_EINVAL
    bad = dict(a, n_clusters=16385)
    assert runtime.monitor_reconcile_check(**bad) == runtime.KAD_EUNSUPPORTED
    bad = dict(a, obj_flags=a["obj_flags"] | M.HAS_LAST)  # NEW with HAS_LAST
    assert runtime.monitor_reconcile_check(**bad) == runtime.KAD_EINVAL
    assert runtime.monitor_report_check(T0, 3, 16) == 0
    assert runtime.monitor_report_check(-5, 3, 16) == runtime.KAD_EINVAL
    assert runtime.monitor_report_check(T0, -1, 16) == runtime.KAD_EINVAL


def test_route_eval():
    r = runtime.monitor_reconcile_route_eval(1000, 0, 3000)
    assert r == dict(width=1, long_min=512, threads=256, grid=4, long_grid=0, stride=1024)
    r = runtime.monitor_reconcile_route_eval(1000, 2, 998 * 100)
    assert (r["width"], r["long_grid"], r["grid"]) == (16, 2, 63)
    assert runtime.monitor_reconcile_route_eval(3, 3, 0)["grid"] == 0
    r = runtime.monitor_report_route_eval(10_000_000, 8)
    assert r == dict(path=0, bins=4096, threads=256, grid=2048, vec=4, wtiles=39063)
    assert runtime.monitor_report_route_eval(0, 8)["grid"] == 0
    assert runtime.monitor_report_route_eval(1025, 8)["grid"] == 2
    at, over = runtime.monitor_report_route_eval(10_000_000, 4096), runtime.monitor_report_route_eval(10_000_000, 4097)
    assert (at["path"], at["grid"]) == (0, 256 * 4) and (over["path"], over["grid"]) == (1, 2048)
    with pytest.raises(runtime.KadError):
        runtime.monitor_report_route_eval(-1, 8)


def test_seeded_generator_is_deterministic():
    from kubeadmiral_amd import synth
    assert synth.gen_monitor_events(3) == synth.gen_monitor_events(3)
    assert synth.gen_monitor_events(3) != synth.gen_monitor_events(4)
