"""The monitor's named cases and seeded batches, and the harness that runs them through the checker (monitor_ref.py)
and through kubeadmiral_amd.monitor on a backend (the numpy restatement or a runtime.Context), comparing everything:
the worker result, the annotation decision, the log line's values, the stored meter, the lastStatus map, the report.

A case: ``seed`` = meters put into the table before the first step (times in Unix ns, None = Go's zero time), ``steps``
= (now in Unix ns, event). Times in events are RFC3339Nano strings."""
import json
import os

import numpy as np

import monitor_ref as R
from kubeadmiral_amd import monitor as M
from kubeadmiral_amd import synth

T0 = 1_700_000_000_000_000_000  # 2023-11-14T22:13:20Z
S, MIN = 10 ** 9, 60 * 10 ** 9
K = "FederatedDeployment/default/web"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "monitor.json")


def stamp(ns):
    import datetime
    s, f = divmod(ns, S)
    base = datetime.datetime.fromtimestamp(s, datetime.timezone.utc).strftime("%Y-%m-%dT%H:%M:%S")
    return base + (("." + ("%09d" % f).rstrip("0")) if f else "") + "Z"


def obj(gen=7, creation=T0 - 3600 * S, sync=None, last_gen=None, lssg=None, deleted=False):
    ann = {}
    if sync is not None:
        ann["syncSuccessTimestamp"] = sync if isinstance(sync, str) else stamp(sync)
    if last_gen is not None:
        ann["lastGeneration"] = last_gen
    if lssg is not None:
        ann["lastSyncSuccessGeneration"] = lssg
    meta = dict(generation=gen, annotations=ann)
    if creation is not None:
        meta["creationTimestamp"] = creation if isinstance(creation, str) else stamp(creation)
    if deleted:
        meta["deletionTimestamp"] = stamp(T0)
    return dict(metadata=meta)


def fed(m):
    return dict(metadata={}, clusterStatus=[dict(clusterName=c, status=dict(observedGeneration=g)) for c, g in m])


def mem(m):
    return [(c, dict(status=dict(observedGeneration=g))) for c, g in m]


def ev(o, status=None, members=(), enabled=True, key=K):
    return dict(key=key, obj=o, status_enabled=enabled, status=status, members=list(members))


def synced_obj(**kw):
    return obj(sync=T0 - 30 * S, last_gen="7", lssg="7", **kw)


def seed(last=None, lst=None, oos=0, creation=T0 - 3600 * S, lu=None, ss=T0 - 1800 * S, key=K):
    return dict(key=key, creation=creation, last_update=lu, sync_success=ss, last_status=last, last_status_synced=lst,
                out_of_sync=oos)


A2 = [("a", 2), ("b", 2)]
A3 = [("a", 3), ("b", 2)]
CASES = {
    "first_visit": dict(steps=[(T0, ev(obj(sync=T0 - 5 * S), fed(A2), mem(A2)))]),
    "synced": dict(steps=[(T0, ev(synced_obj(), fed(A2), mem(A2))), (T0 + 10 * S, ev(synced_obj(), fed(A2), mem(A2)))]),
    "out_of_sync_last_unchanged": dict(seed=[seed(dict(A3), T0 - 400 * S, 0)],
                                       steps=[(T0, ev(synced_obj(), fed(A2), mem(A3)))]),
    "out_of_sync_last_changed_zero": dict(seed=[seed(dict(A2), T0 - 400 * S, 0)],
                                          steps=[(T0, ev(synced_obj(), fed(A2), mem(A3)))]),
    "out_of_sync_last_changed_nonzero": dict(seed=[seed(dict(A2), T0 - 400 * S, 7 * MIN)],
                                             steps=[(T0, ev(synced_obj(), fed(A2), mem(A3)))]),
    "out_of_sync_meter_untouched": dict(seed=[seed(dict(A2), T0 - 900 * S, 11 * MIN)],
                                        steps=[(T0, ev(synced_obj(), fed(A2), mem(A3))),
                                               (T0 + 5 * S, ev(synced_obj(), fed(A2), mem(A3)))]),
    "nil_last_status": dict(seed=[seed(None, None, 0)], steps=[(T0, ev(synced_obj(), fed(A2), mem([])))]),
    "empty_last_status": dict(seed=[seed({}, T0 - 400 * S, 0)], steps=[(T0, ev(synced_obj(), fed(A2), mem([])))]),
    "empty_equals_empty": dict(seed=[seed({}, T0 - 400 * S, 9 * MIN)], steps=[(T0, ev(synced_obj(), fed([]), mem([])))]),
    "fed_missing_before_cluster_error": dict(steps=[(T0, ev(synced_obj(), dict(metadata={}, clusterStatus=[
        dict(clusterName="a", status={})]), [("a", dict(status={}))]))]),
    "fed_missing_name": dict(steps=[(T0, ev(synced_obj(), dict(metadata={}, clusterStatus=[
        dict(status=dict(observedGeneration=1))]), mem(A2)))]),
    "cluster_error": dict(steps=[(T0, ev(synced_obj(), fed(A2), [("a", dict(status=dict(observedGeneration=2))), ("b", dict())]))]),
    "duplicate_fed_names": dict(seed=[seed(dict(A3), T0 - 400 * S, 0)],
                                steps=[(T0, ev(synced_obj(), fed([("a", 2), ("b", 2), ("a", 3)]), mem(A3)))]),
    "status_absent": dict(steps=[(T0, ev(synced_obj(), None, mem(A2)))]),
    "status_deleted": dict(steps=[(T0, ev(synced_obj(), dict(metadata=dict(deletionTimestamp=stamp(T0)), clusterStatus=[]), mem(A2)))]),
    "status_disabled": dict(steps=[(T0, ev(synced_obj(), fed(A2), mem(A3), enabled=False))]),
    "deleted": dict(seed=[seed(dict(A2), T0 - 400 * S, 0)], steps=[(T0, ev(synced_obj(deleted=True))), (T0 + S, ev(None))]),
    "absent_unknown": dict(steps=[(T0, ev(None))]),
    "no_creation_timestamp": dict(steps=[(T0, ev(obj(creation=None, sync=T0 - 5 * S), fed(A2), mem(A2)))]),
    "unparsable_creation_timestamp": dict(steps=[(T0, ev(obj(creation="last week", sync=T0 - 5 * S), fed(A2), mem(A2)))]),
    "no_sync_annotation": dict(steps=[(T0, ev(obj(last_gen="7"), fed(A2), mem(A2)))]),
    "unparsable_sync_keeps_previous": dict(seed=[seed(None, None, 0, ss=T0 - 20 * S)],
                                           steps=[(T0, ev(obj(sync="soon", last_gen="7"), fed(A2), mem(A2)))]),
    "minus_10ms_from_zero_sync": dict(steps=[(T0, ev(obj(last_gen="6", lssg="7"), fed(A2), mem(A2)))]),
    "minus_10ms_from_real_sync": dict(steps=[(T0, ev(obj(sync=T0 - 5 * S, last_gen="6", lssg="7"), fed(A2), mem(A2)))]),
    "race_adjustment": dict(seed=[seed(None, None, 0, lu=T0 - 10 * S, ss=T0 - 20 * S)],
                            steps=[(T0, ev(obj(sync=T0 - 15 * S, last_gen="7", lssg="7"), fed(A2), mem(A2)))]),
    "zero_padded_generation": dict(steps=[(T0, ev(obj(sync=T0 - 5 * S, last_gen="07", lssg="07"), fed(A2), mem(A2)))]),
    "generation_changed_no_lssg": dict(steps=[(T0, ev(obj(sync=T0 - 5 * S, last_gen="6"), fed(A2), mem(A2)))]),
    "nine_digit_fraction_offset": dict(steps=[(T0, ev(obj(sync="2023-11-15T06:13:15.123456789+08:00", last_gen="7"), fed(A2), mem(A2)))]),
    "late_sync_buckets": dict(seed=[seed(None, None, 0, creation=T0 - 7 * MIN, lu=T0 - 6 * MIN, ss=T0 - 8 * MIN),
                                    seed(None, None, 0, creation=T0 - 2 * 86400 * S, ss=None, key="FederatedJob/default/old")],
                              steps=[(T0, ev(None, key="FederatedJob/default/none"))]),
}


def dev_time(t):
    """A checker time (ns since year 1) as the device holds it."""
    return M.TIME_ZERO + t if abs(t) < (1 << 60) else t - R.EPOCH


class NumpyBackend:
    """kubeadmiral_amd.monitor's numpy restatements on a Mirror of its own."""

    def __init__(self, table):
        self.table = table
        self.mirror = M.Mirror()

    def run(self, **a):
        return M.reconcile_numpy(self.mirror, **a)

    def reserve(self, cap):
        self.mirror.ensure(cap)

    def load(self, slots, type_id, flags, **cols):
        m = self.mirror
        m.ensure(max(slots) + 1)
        for k, v in cols.items():
            m.cols[M.COLUMNS.index(k), slots] = v
        m.type_id[slots], m.flags[slots] = type_id, flags
        m.n_slots = max(m.n_slots, max(slots) + 1)

    def read(self, slots):
        m = self.mirror
        return {**{k: m.cols[i, slots] for i, k in enumerate(M.COLUMNS)}, "type_id": m.type_id[slots], "flags": m.flags[slots]}

    def report(self, now, n_types):
        return M.report_numpy(self.mirror, now, n_types)


class DeviceBackend:
    """A runtime.Context; ``width`` / ``long_min`` forced on every reconcile."""

    def __init__(self, ctx, width=0, long_min=0):
        self.ctx, self.width, self.long_min = ctx, width, long_min
        ctx.monitor_clear()

    def run(self, **a):
        self.ctx.monitor_reconcile_debug_route(self.width, self.long_min)
        try:
            return self.ctx.monitor_reconcile(**a)
        finally:
            self.ctx.monitor_reconcile_debug_route(0, 0)

    def reserve(self, cap):
        self.ctx.monitor_reserve(cap)

    def load(self, slots, type_id, flags, **cols):
        self.ctx.monitor_reserve(max(slots) + 1)
        self.ctx.monitor_load(slots, type_id=type_id, flags=flags, **cols)

    def read(self, slots):
        return self.ctx.monitor_read(slots)

    def report(self, now, n_types):
        return self.ctx.monitor_report(now, n_types)


class Harness:
    """The checker and a MeterTable on a backend, side by side."""

    def __init__(self, make_backend):
        self.ref = R.Monitor()
        self.table = M.MeterTable()
        self.be = make_backend(self.table)

    def seed(self, seeds):
        slots, types, cols = [], [], [[] for _ in M.COLUMNS]
        for s in seeds:
            m = R.Meter()
            for f in ("creation", "last_update", "sync_success", "last_status_synced"):
                setattr(m, f, 0 if s[f] is None else R.unix(s[f]))
            m.out_of_sync = s["out_of_sync"]
            m.last_status = None if s["last_status"] is None else dict(s["last_status"])
            self.ref.meters[s["key"]] = m
            slot = self.table.acquire(s["key"])
            if m.last_status is not None:
                pairs = sorted((self.table.cluster_id(c), g) for c, g in m.last_status.items())
                self.table.last[slot] = (np.array([p[0] for p in pairs], np.int32), np.array([p[1] for p in pairs], np.int64))
            slots.append(slot)
            types.append(self.table.kind_id(s["key"]))
            for c, v in zip(cols, (dev_time(m.creation), dev_time(m.last_update), dev_time(m.sync_success),
                                   dev_time(m.last_status_synced), m.out_of_sync)):
                c.append(v)
        if slots:  # one load for all of them
            self.be.load(slots, types, [M.LIVE] * len(slots), **dict(zip(M.COLUMNS, cols)))

    def step(self, now, events):
        """The events through both; returns the first difference as a string, or None."""
        want = [self.ref.reconcile(e, R.unix(now)) for e in events]
        got = self.table.reconcile(events, now, self.be.run, self.be.reserve)
        for e, w, g in zip(events, want, got):
            a = (w["result"], w["requeue"], w["update"], w["last_generation"], w["deleted"], w["stored"], w["missing"])
            b = (g.result, g.requeue_after_s, g.update_annotation, g.last_generation, g.meter_deleted, g.status_stored,
                 g.missing_observed_generation)
            if a != b:
                return f"{e['key']}: outcome {b} != {a}"
            if w["log"] is not None:
                a = (w["log"][0], dev_time(w["log"][1]), w["log"][2])
                b = (g.log_last_status, g.log_last_status_synced, g.log_out_of_sync_ns)
                if a != b:
                    return f"{e['key']}: log line {b} != {a}"
        return self.state_diff()

    def state_diff(self):
        """Every meter of the checker against the backend's table and the lastStatus store."""
        if set(self.ref.meters) != set(self.table.slot_of):
            return f"keys {sorted(self.table.slot_of)} != {sorted(self.ref.meters)}"
        if not self.ref.meters:
            return None
        keys = sorted(self.ref.meters, key=self.table.slot_of.get)
        slots = [self.table.slot_of[k] for k in keys]
        rd = self.be.read(slots)
        names = self.table.cluster_names
        for i, k in enumerate(keys):
            m = self.ref.meters[k]
            a = (dev_time(m.creation), dev_time(m.last_update), dev_time(m.sync_success), dev_time(m.last_status_synced),
                 m.out_of_sync, self.table.kinds[k.split("/")[0]], M.LIVE)
            b = tuple(int(rd[c][i]) for c in M.COLUMNS) + (int(rd["type_id"][i]), int(rd["flags"][i]))
            if a != b:
                return f"{k}: stored meter {b} != {a}"
            ls = self.table.last.get(slots[i])
            ls = None if ls is None else {names[c]: int(g) for c, g in zip(*ls)}
            if ls != m.last_status:
                return f"{k}: lastStatus {ls} != {m.last_status}"
        return None

    def report_diff(self, now):
        r = self.be.report(now, self.table.n_types)
        if list(r["sync_slot"]) != sorted(r["sync_slot"]) or list(r["status_slot"]) != sorted(r["status_slot"]):
            return "timer lists are not in ascending slot order"
        w = self.ref.report(R.unix(now))
        for name, lst in (("sync", list(zip(r["sync_slot"], r["sync_ms"]))), ("status", list(zip(r["status_slot"], r["status_ms"])))):
            want = sorted((self.table.slot_of[k], v) for k, v in w[name + "_timers"].items())
            if [(int(s), int(v)) for s, v in lst] != want:
                return f"{name} timers {lst} != {want}"
        got = sorted(M.Report.from_result(self.table, r).to_metrics())
        want = self.ref.metrics(R.unix(now))
        if got != want:
            return f"metrics {[x for x in got if x not in want]} != {[x for x in want if x not in got]}"
        return None


def run_case(case, make_backend):
    """A named case through a harness: the first difference, or None. Reports after every step at the step's time
    and at every bucket boundary past it."""
    h = Harness(make_backend)
    h.seed(case.get("seed", ()))
    for now, e in case["steps"]:
        d = h.step(now, [e]) or h.report_diff(now) or h.report_diff(now + 61 * S)
        if d:
            return d
    return None


def run_seeded(seed, make_backend, **kw):
    h = Harness(make_backend)
    for now, events in synth.gen_monitor_events(seed, **kw):
        d = h.step(now, events) or h.report_diff(now) or h.report_diff(now + 6 * MIN)
        if d:
            return f"seed {seed}: {d}"
    return None


def golden():
    """The named cases with the checker's outputs (tests/golden/monitor.json holds them)."""
    out = {}
    for name, case in CASES.items():
        h = Harness(NumpyBackend)
        h.seed(case.get("seed", ()))
        steps = []
        for now, e in case["steps"]:
            w = h.ref.reconcile(e, R.unix(now))
            h.table.reconcile([e], now, h.be.run, h.be.reserve)
            w["log"] = None if w["log"] is None else [w["log"][0], dev_time(w["log"][1]), w["log"][2]]
            steps.append(dict(now=now, outcome=w, metrics=[list(m[:3]) + [list(map(list, m[3]))] for m in h.ref.metrics(R.unix(now))]))
        out[name] = steps
    return out


if __name__ == "__main__":  # python tests/monitor_cases.py: rewrite the golden file from the checker
    with open(GOLDEN, "w") as f:
        json.dump(golden(), f, indent=1, sort_keys=True)
        f.write("\n")
