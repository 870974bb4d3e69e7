"""The monitor controller's host half (pkg/controllers/monitor): meter keys to slots, strings to flags, the
lastStatus maps, and the report as the metrics report.go emits.

The meters' numbers live on the device (kad_monitor_*, include/kad_sched.h); this module keeps what the device never
sees: the key of every slot, the interned kinds and cluster names, and each meter's ``lastStatus`` map, which the
device only says when to replace. ``reconcile_numpy`` / ``report_numpy`` restate both calls on a numpy copy of the
table (a ``Mirror`` that tests and measurements build for themselves; nothing on the product path keeps or reads
one, and there is no CPU fallback).

An event is a dict: ``key`` (the meter key, ``<Kind>/<namespace>/<name>``), ``obj`` (the federated object as the
informer holds it, None when absent), ``status_enabled`` (the type config's), ``status`` (the status object, None when
absent) and ``members`` (a list of (cluster name, the member cluster's object)).

Time: int64 nanoseconds since the Unix epoch; Go's zero time is ``TIME_ZERO`` (kad_monitor.h). A timestamp outside
[1970, 2116) other than the zero time itself is rejected (declared deviation: the reference accepts years 0-9999).
"""

from __future__ import annotations

import heapq
import re
from dataclasses import dataclass, field
from typing import Callable, Dict, List, Optional, Sequence, Tuple

import numpy as np

TIME_ZERO = -(1 << 62)
_NEAR = -(1 << 61)
_TIME_END = 1 << 62
_GO_ZERO_UNIX_NS = -62135596800 * 10 ** 9  # 0001-01-01T00:00:00Z
MS, SECOND, MINUTE = 10 ** 6, 10 ** 9, 60 * 10 ** 9
REPORT_INTERVAL = MINUTE
REQUEUE_SECONDS = 5  # OutOfSyncRecheckDelay
I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1
BUCKETS = (("latency5min", 5), ("latency10min", 10), ("latency30min", 30), ("latency1hour", 60), ("latency6hour", 180),
           ("latency1day", 1440))
COLUMNS = ("creation", "last_update", "sync_success", "last_status_synced", "out_of_sync_ns")
CR, LU, SS, LST, OOS = range(5)

DELETED, NEW, SS_PARSED, LASTGEN_PRESENT, LASTGEN_EQUAL, LSSG_PRESENT, LSSG_EQUAL, STATUS_ENABLED, STATUS_ABSENT, \
    FED_MISSING, CLUSTER_ERR, HAS_LAST = (1 << i for i in range(12))
ALL_OK, STATUS_ERROR, REQUEUE = 0, 1, 2
METER_DELETED, UPDATE_ANNOTATION, STATUS_STORED, REPLACE_LAST, MISSING_OBSERVED_GENERATION, LOG_LAST_CLUSTER = \
    (1 << i for i in range(6))
LIVE = 1
RESULT_NAMES = ("ALL_OK", "ERROR", "REQUEUE")

_RFC3339 = re.compile(r"([0-9]{4})-([0-9]{2})-([0-9]{2})T([0-9]{2}):([0-9]{2}):([0-9]{2})(?:[.,]([0-9]+))?"
                      r"(Z|[+-][0-9]{2}:[0-9]{2})")
_MDAYS = (31, 28, 31, 30, 31, 30, 31, 31, 30, 31, 30, 31)


def _days_from_civil(y: int, m: int, d: int) -> int:
    y -= m <= 2
    era = y // 400
    yoe = y - era * 400
    doy = (153 * (m + (-3 if m > 2 else 9)) + 2) // 5 + d - 1
    return era * 146097 + yoe * 365 + yoe // 4 - yoe // 100 + doy - 719468


def parse_rfc3339nano(s) -> Optional[int]:
    """time.Parse(time.RFC3339Nano, s) as nanoseconds since the Unix epoch (a Python int, any year 0-9999), or None
    where the Go returns an error. The fraction may have any number of digits (those past the ninth are dropped, as
    the Go does); the zone is ``Z`` or ``±hh:mm``."""
    m = _RFC3339.fullmatch(s) if isinstance(s, str) else None
    if m is None:
        return None
    y, mo, d, h, mi, sec = (int(x) for x in m.groups()[:6])
    leap = y % 4 == 0 and (y % 100 != 0 or y % 400 == 0)
    if not 1 <= mo <= 12 or not 1 <= d <= _MDAYS[mo - 1] + (mo == 2 and leap) or h > 23 or mi > 59 or sec > 59:
        return None
    frac = int((m.group(7) or "0")[:9].ljust(9, "0"))
    off = 0
    z = m.group(8)
    if z != "Z":
        zh, zm = int(z[1:3]), int(z[4:6])
        if zh > 23 or zm > 59:
            return None
        off = (zh * 3600 + zm * 60) * (1 if z[0] == "+" else -1)
    return ((_days_from_civil(y, mo, d) * 86400 + h * 3600 + mi * 60 + sec - off) * SECOND) + frac


def device_time(unix_ns: Optional[int]) -> int:
    """A parsed time as the device holds it: None (no timestamp) and Go's zero time are TIME_ZERO."""
    if unix_ns is None or unix_ns == _GO_ZERO_UNIX_NS:
        return TIME_ZERO
    if not 0 <= unix_ns < _TIME_END:
        raise ValueError(f"timestamp {unix_ns} ns is outside the device's range [1970, 2116)")
    return unix_ns


def sat_sub(a: int, b: int) -> int:
    """Time.Sub on device times (Python ints)."""
    if (a < _NEAR) != (b < _NEAR):
        return I64_MIN if a < _NEAR else I64_MAX
    return a - b


def _trunc_div(d: int, m: int) -> int:
    return -((-d) // m) if d < 0 else d // m


class Mirror:
    """A numpy copy of the device table."""

    def __init__(self):
        self.cols = np.zeros((5, 0), np.int64)
        self.type_id = np.zeros(0, np.int32)
        self.flags = np.zeros(0, np.uint8)
        self.n_slots = 0

    def ensure(self, cap: int) -> None:
        if cap > self.cols.shape[1]:
            grow = max(cap, 2 * self.cols.shape[1], 64) - self.cols.shape[1]  # doubling: appends are amortised
            self.cols = np.concatenate([self.cols, np.zeros((5, grow), np.int64)], axis=1)
            self.type_id = np.concatenate([self.type_id, np.zeros(grow, np.int32)])
            self.flags = np.concatenate([self.flags, np.zeros(grow, np.uint8)])

    def clear(self) -> None:
        self.flags[:] = 0
        self.n_slots = 0


@dataclass
class MonitorOutcome:
    """What the reference's worker does with one event."""
    result: str                    # ALL_OK, ERROR, REQUEUE
    requeue_after_s: Optional[int]  # 5 with REQUEUE
    update_annotation: bool        # write the lastGeneration annotation ...
    last_generation: Optional[str]  # ... with this value
    meter_deleted: bool = False
    status_stored: bool = False
    missing_observed_generation: bool = False
    meter: Optional[Tuple[int, ...]] = None  # the stored meter's five values after the call
    log_last_status_synced: Optional[int] = None  # the log line's values (would-be on REQUEUE)
    log_out_of_sync_ns: Optional[int] = None
    log_last_status: Optional[Dict[str, int]] = None


class LastStore:
    """The meters' lastStatus maps in CSR form: one pool of (cluster id, generation) entries and per slot where its
    list starts and how long it is (-1: nil, which an empty list is not). A replaced list is appended and the old
    entries become garbage; the pool is compacted once more than half of it is. Reads like a mapping slot → (ids
    ascending, generations), both views into the pool that the next write may invalidate."""

    def __init__(self):
        self.clear()

    def clear(self) -> None:
        self.start = np.zeros(0, np.int64)
        self.length = np.zeros(0, np.int64)  # -1: no lastStatus
        self.cluster = np.zeros(64, np.int32)
        self.gen = np.zeros(64, np.int64)
        self.used = 0     # pool entries written
        self.garbage = 0  # of them no longer referenced

    def __contains__(self, slot: int) -> bool:
        return 0 <= slot < len(self.length) and self.length[slot] >= 0

    def __getitem__(self, slot: int) -> Tuple[np.ndarray, np.ndarray]:
        if slot not in self:
            raise KeyError(slot)
        lo, n = int(self.start[slot]), int(self.length[slot])
        return self.cluster[lo:lo + n], self.gen[lo:lo + n]

    def get(self, slot: int, default=None):
        return self[slot] if slot in self else default

    def pop(self, slot: int, default=None):
        if slot in self:
            self.garbage += int(self.length[slot])
            self.length[slot] = -1
        return default

    def __setitem__(self, slot: int, value) -> None:
        ids, gens = (np.asarray(value[0], np.int32), np.asarray(value[1], np.int64))
        n = len(ids)
        if slot >= len(self.length):
            grow = max(slot + 1, 2 * len(self.length), 64) - len(self.length)
            self.start = np.concatenate([self.start, np.zeros(grow, np.int64)])
            self.length = np.concatenate([self.length, np.full(grow, -1, np.int64)])
        self.pop(slot)
        if self.garbage > 1024 and 2 * self.garbage > self.used:
            self._compact()
        if self.used + n > len(self.cluster):
            cap = max(self.used + n, 2 * len(self.cluster))
            self.cluster = np.concatenate([self.cluster[:self.used], np.zeros(cap - self.used, np.int32)])
            self.gen = np.concatenate([self.gen[:self.used], np.zeros(cap - self.used, np.int64)])
        self.cluster[self.used:self.used + n] = ids
        self.gen[self.used:self.used + n] = gens
        self.start[slot], self.length[slot] = self.used, n
        self.used += n

    def _compact(self) -> None:
        live = np.nonzero(self.length > 0)[0]
        n = self.length[live]
        new_start = np.concatenate([[0], np.cumsum(n)])[:-1] if len(live) else np.zeros(0, np.int64)
        idx = np.repeat(self.start[live] - new_start, n) + np.arange(int(n.sum()))
        self.cluster, self.gen = self.cluster[idx].copy(), self.gen[idx].copy()
        self.start[live] = new_start
        self.used, self.garbage = int(n.sum()), 0
        if len(self.cluster) < 64:
            self.cluster = np.concatenate([self.cluster, np.zeros(64, np.int32)])
            self.gen = np.concatenate([self.gen, np.zeros(64, np.int64)])


class MeterTable:
    """Meter keys to slots (lowest free slot first), interned kinds and cluster names, the lastStatus store."""

    def __init__(self):
        self.slot_of: Dict[str, int] = {}
        self.key_of: Dict[int, str] = {}
        self._free: List[int] = []
        self._next = 0
        self.kinds: Dict[str, int] = {}
        self.clusters: Dict[str, int] = {}
        self.last = LastStore()  # slot → (cluster ids ascending, generations)

    @property
    def capacity_needed(self) -> int:
        return self._next

    @property
    def n_types(self) -> int:
        return max(1, len(self.kinds))

    @property
    def kind_names(self) -> List[str]:
        return sorted(self.kinds, key=self.kinds.get)

    @property
    def cluster_names(self) -> List[str]:
        return sorted(self.clusters, key=self.clusters.get)

    def kind_id(self, key: str) -> int:
        return self.kinds.setdefault(key.split("/")[0], len(self.kinds))

    def cluster_id(self, name: str) -> int:
        return self.clusters.setdefault(name, len(self.clusters))

    def acquire(self, key: str) -> int:
        slot = heapq.heappop(self._free) if self._free else self._next
        if slot == self._next:
            self._next += 1
        self.slot_of[key] = slot
        self.key_of[slot] = key
        return slot

    def release(self, key: str) -> None:
        slot = self.slot_of.pop(key)
        del self.key_of[slot]
        self.last.pop(slot, None)
        heapq.heappush(self._free, slot)

    def clear(self) -> None:
        self.slot_of.clear()
        self.key_of.clear()
        self.last.clear()
        self._free, self._next = [], 0

    @staticmethod
    def split(events: Sequence[dict]) -> List[List[int]]:
        """The events' indices in successive calls, none of which repeats a key (the reference's worker serialises
        per key): an event goes to the call after the last earlier event of its key."""
        calls: List[List[int]] = []
        at: Dict[str, int] = {}
        for i, e in enumerate(events):
            k = at.get(e["key"], -1) + 1
            at[e["key"]] = k
            if k == len(calls):
                calls.append([])
            calls[k].append(i)
        return calls

    def reconcile(self, events: Sequence[dict], now_ns: int, run: Callable[..., dict],
                  reserve: Optional[Callable[[int], None]] = None) -> List[MonitorOutcome]:
        """Every event through ``run`` (Context.monitor_reconcile, or reconcile_numpy bound to a Mirror), a key's
        events in successive calls. ``reserve(capacity)`` is called before a call that needs more slots."""
        out: List[Optional[MonitorOutcome]] = [None] * len(events)
        for idx in self.split(events):
            batch = MonitorBatch.pack(self, [events[i] for i in idx], now_ns)
            try:
                if reserve is not None:
                    reserve(self.capacity_needed)
                result = run(**batch.arrays()) if batch.n else None
            except BaseException:
                batch.rollback()  # the call did not happen: the slots it would have started are free again
                raise
            for i, o in zip(idx, batch.apply(result)):
                out[i] = o
        return out  # type: ignore[return-value]


def _fed_list(status: dict) -> Optional[Dict[str, int]]:
    """getFedStatusObservedGeneration (:383-404): None for ErrMissingObservedGenerationField."""
    entries = status.get("clusterStatus")
    ret: Dict[str, int] = {}
    for e in entries if isinstance(entries, list) else ():
        if e is None or e.get("clusterName") is None:
            return None
        name = e["clusterName"]
        if not isinstance(name, str):
            raise TypeError("clusterStatus[].clusterName is not a string (the reference panics)")
        st = e.get("status")
        if st is not None and not isinstance(st, dict):
            raise TypeError("clusterStatus[].status is not an object (the reference panics)")
        if st is None or st.get("observedGeneration") is None:
            return None
        g = st["observedGeneration"]
        if isinstance(g, bool) or not isinstance(g, int) or not I64_MIN <= g <= I64_MAX:
            raise TypeError("clusterStatus[].status.observedGeneration is not an int64 (the reference panics)")
        ret[name] = g  # a later entry of the same name wins
    return ret


def _member_list(members) -> Optional[Dict[str, int]]:
    """getClusterObservedGeneration (:407-433): None where NestedInt64 fails."""
    ret: Dict[str, int] = {}
    for name, obj in members or ():
        st = obj.get("status") if isinstance(obj, dict) else None
        g = st.get("observedGeneration") if isinstance(st, dict) else None
        if isinstance(g, bool) or not isinstance(g, int) or not I64_MIN <= g <= I64_MAX:
            return None
        ret[name] = g
    return ret


class MonitorBatch:
    """One kad_monitor_reconcile call: events with distinct keys as the call's arrays."""

    @classmethod
    def pack(cls, table: MeterTable, events: Sequence[dict], now_ns: int) -> "MonitorBatch":
        b = cls()
        b.table, b.now_ns = table, int(now_ns)
        b.events = list(events)
        if len({e["key"] for e in b.events}) != len(b.events):
            raise ValueError("MonitorBatch.pack: a key repeats (MeterTable.split / reconcile serialise per key)")
        b.sent: List[int] = []          # the events the device sees
        b.acquired: List[str] = []      # the keys that got a slot here (rollback)
        b.gen_str: List[Optional[str]] = []
        b.mem: List[Optional[Dict[str, int]]] = []
        slot, flags, type_id, creation, sync_success = [], [], [], [], []
        lists: Tuple[list, list, list] = ([], [], [])  # fed, mem, last per sent event: (ids, gens)
        empty = (np.zeros(0, np.int32), np.zeros(0, np.int64))
        for i, e in enumerate(b.events):
            key, obj = e["key"], e.get("obj")
            known = key in table.slot_of
            gone = obj is None or obj.get("metadata", {}).get("deletionTimestamp") is not None
            b.gen_str.append(None)
            b.mem.append(None)
            if gone and not known:
                continue  # meters.Delete of an absent key
            b.sent.append(i)
            f = 0
            cr = ss = TIME_ZERO
            fed = mem = empty
            if gone:
                f = DELETED
                s = table.slot_of[key]
            else:
                meta = obj.get("metadata", {})
                ann = meta.get("annotations") or {}
                s = table.slot_of[key] if known else table.acquire(key)
                if not known:
                    b.acquired.append(key)
                    f |= NEW
                    cr = device_time(parse_rfc3339nano(meta.get("creationTimestamp")))
                if "syncSuccessTimestamp" in ann:
                    t = parse_rfc3339nano(ann["syncSuccessTimestamp"])
                    if t is not None:
                        f |= SS_PARSED
                        ss = device_time(t)
                gen = str(int(meta.get("generation", 0)))
                b.gen_str[i] = gen
                if "lastGeneration" in ann:
                    f |= LASTGEN_PRESENT | (LASTGEN_EQUAL if ann["lastGeneration"] == gen else 0)
                if "lastSyncSuccessGeneration" in ann:
                    f |= LSSG_PRESENT | (LSSG_EQUAL if ann["lastSyncSuccessGeneration"] == gen else 0)
                if s in table.last:
                    f |= HAS_LAST
                if e.get("status_enabled"):
                    f |= STATUS_ENABLED
                    status = e.get("status")
                    if status is None or status.get("metadata", {}).get("deletionTimestamp") is not None:
                        f |= STATUS_ABSENT
                    else:
                        fm = _fed_list(status)
                        mm = None if fm is None else _member_list(e.get("members"))
                        if fm is None:
                            f |= FED_MISSING
                        elif mm is None:
                            f |= CLUSTER_ERR
                        else:
                            fed, mem = b._ids(fm), b._ids(mm)
                            b.mem[i] = mm
            slot.append(s)
            flags.append(f)
            type_id.append(table.kind_id(key))
            creation.append(cr)
            sync_success.append(ss)
            lists[0].append(fed)
            lists[1].append(mem)
            lists[2].append(table.last.get(s, empty) if not gone else empty)
        b.n = len(b.sent)
        b._arrays = dict(n_clusters=max(1, len(table.clusters)), now_ns=b.now_ns, slot=np.array(slot, np.int32),
                         obj_flags=np.array(flags, np.uint16), type_id=np.array(type_id, np.int32),
                         creation_ns=np.array(creation, np.int64), sync_success_ns=np.array(sync_success, np.int64))
        for name, ls in zip(("fed", "mem", "last"), lists):
            b._arrays[name + "_off"] = np.concatenate([[0], np.cumsum([len(x[0]) for x in ls])]).astype(np.int32)
            b._arrays[name + "_cluster"] = np.concatenate([x[0] for x in ls] + [empty[0]]).astype(np.int32)
            b._arrays[name + "_gen"] = np.concatenate([x[1] for x in ls] + [empty[1]]).astype(np.int64)
        return b

    def _ids(self, m: Dict[str, int]) -> Tuple[np.ndarray, np.ndarray]:
        pairs = sorted((self.table.cluster_id(k), g) for k, g in m.items())
        return np.array([p[0] for p in pairs], np.int32), np.array([p[1] for p in pairs], np.int64)

    def rollback(self) -> None:
        """The call failed or was never made: the slots pack took for new keys go back to the free list, so that
        their keys are new again. Interned kinds and cluster names stay: an id nobody uses is harmless."""
        for key in self.acquired:
            if key in self.table.slot_of:
                self.table.release(key)
        self.acquired = []

    def arrays(self) -> dict:
        """The keyword arguments of Context.monitor_reconcile / reconcile_numpy."""
        return self._arrays

    def apply(self, result: Optional[dict]) -> List[MonitorOutcome]:
        """The call's outputs into the table (freed slots, replaced lastStatus maps) → one outcome per event of
        the batch."""
        t = self.table
        out = [MonitorOutcome("ALL_OK", None, False, None, meter_deleted=True) for _ in self.events]
        names = t.cluster_names
        for j, i in enumerate(self.sent):
            e = self.events[i]
            res, bits = int(result["result"][j]), int(result["bits"][j])
            s = int(self._arrays["slot"][j])
            if bits & METER_DELETED:
                t.release(e["key"])
                continue
            if bits & REPLACE_LAST:
                lo, hi = self._arrays["mem_off"][j], self._arrays["mem_off"][j + 1]
                t.last[s] = (self._arrays["mem_cluster"][lo:hi], self._arrays["mem_gen"][lo:hi])
            meter = tuple(int(x) for x in result["meter"][j])
            if bits & LOG_LAST_CLUSTER:
                log_last = dict(self.mem[i] or {})
            elif s in t.last and not bits & REPLACE_LAST:
                log_last = {names[c]: int(g) for c, g in zip(*t.last[s])}
            else:
                log_last = None
            upd = bool(bits & UPDATE_ANNOTATION)
            out[i] = MonitorOutcome(RESULT_NAMES[res], REQUEUE_SECONDS if res == REQUEUE else None, upd,
                                    self.gen_str[i] if upd else None, False, bool(bits & STATUS_STORED),
                                    bool(bits & MISSING_OBSERVED_GENERATION), meter, int(result["would"][j][0]),
                                    int(result["would"][j][1]), log_last)
        return out


def reconcile_numpy(mirror: Mirror, n_clusters: int, now_ns: int, **a) -> dict:
    """kad_monitor_reconcile restated on ``mirror`` (which it updates): the same outputs."""
    n = len(a["obj_flags"])
    out = dict(result=np.zeros(n, np.uint8), bits=np.zeros(n, np.uint8), meter=np.zeros((n, 5), np.int64),
               would=np.zeros((n, 2), np.int64))
    now = int(now_ns)

    def lst_of(name, i):
        lo, hi = a[name + "_off"][i], a[name + "_off"][i + 1]
        return a[name + "_cluster"][lo:hi], a[name + "_gen"][lo:hi]

    def equal(x, y):
        return len(x[0]) == len(y[0]) and bool((x[0] == y[0]).all()) and bool((x[1] == y[1]).all())

    for i in range(n):
        f, s = int(a["obj_flags"][i]), int(a["slot"][i])
        mirror.ensure(s + 1)
        if f & DELETED:
            mirror.flags[s] = 0
            out["bits"][i] = METER_DELETED
            continue
        if f & NEW:
            cr, lu, ss, lst, oos = int(a["creation_ns"][i]), TIME_ZERO, TIME_ZERO, TIME_ZERO, 0
        else:
            cr, lu, ss, lst, oos = (int(x) for x in mirror.cols[:, s])
        if f & SS_PARSED:
            ss = int(a["sync_success_ns"][i])
        update = True
        lssg = bool(f & LSSG_PRESENT) and bool(f & LSSG_EQUAL)
        if f & LASTGEN_PRESENT:
            if not f & LASTGEN_EQUAL:
                lu = ss - 10 * MS if lssg else now
            else:
                if lssg and lu > ss:
                    lu = ss - 10 * MS
                update = False
        bits, res, stored = (UPDATE_ANNOTATION if update else 0), ALL_OK, False
        st_lst, st_oos = lst, oos
        if f & STATUS_ENABLED and not f & STATUS_ABSENT:
            if f & FED_MISSING:
                bits |= MISSING_OBSERVED_GENERATION
            elif f & CLUSTER_ERR:
                res = STATUS_ERROR
            elif not f & HAS_LAST:
                lst, stored = now, True
                bits |= LOG_LAST_CLUSTER
            elif equal(lst_of("mem", i), lst_of("fed", i)):
                oos, lst, stored = 0, now, True
                bits |= LOG_LAST_CLUSTER
            else:
                if equal(lst_of("last", i), lst_of("mem", i)):
                    oos = sat_sub(now, lst)
                else:
                    if oos == 0:
                        oos, lst = SECOND, now
                    else:
                        oos = sat_sub(now, lst)
                    bits |= LOG_LAST_CLUSTER
                res = REQUEUE
        out["would"][i] = (lst, oos)
        if stored:
            bits |= STATUS_STORED | REPLACE_LAST
        else:
            lst, oos = st_lst, st_oos
        mirror.cols[:, s] = (cr, lu, ss, lst, oos)
        mirror.type_id[s] = a["type_id"][i]
        mirror.flags[s] = LIVE
        mirror.n_slots = max(mirror.n_slots, s + 1)
        out["meter"][i] = (cr, lu, ss, lst, oos)
        out["result"][i], out["bits"][i] = res, bits
    return out


def report_numpy(mirror: Mirror, now_ns: int, n_types: int) -> dict:
    """kad_monitor_report restated on ``mirror``, vectorised: the same outputs."""
    n, now = mirror.n_slots, np.int64(now_ns)
    cr, lu, ss, lst, oos = (mirror.cols[k, :n] for k in range(5))
    live = (mirror.flags[:n] & LIVE) != 0
    ty = mirror.type_id[:n]
    start = np.where(lu > cr, lu, cr)
    late = live & (start > ss)
    counters = np.zeros(14, np.int32)
    type_sync = np.zeros(n_types, np.int32)
    type_status = np.zeros(n_types, np.int32)
    for b, (_, minutes) in enumerate(BUCKETS):
        d = np.int64(minutes * MINUTE)
        s, t = late & (now > start + d), late & (oos > d)
        counters[b], counters[6 + b] = s.sum(), t.sum()
        if b == 0:
            type_sync[:] = np.bincount(ty[s], minlength=n_types)[:n_types]
            type_status[:] = np.bincount(ty[t], minlength=n_types)[:n_types]
    t_sync = live & (ss + np.int64(REPORT_INTERVAL) > now) & (ss > start)
    t_stat = live & (lst != TIME_ZERO) & (oos > REPORT_INTERVAL)
    counters[12], counters[13] = t_sync.sum(), t_stat.sum()

    def ms(d):
        q = d // MS
        return q + ((d % MS != 0) & (d < 0))

    a, b = ss[t_sync], start[t_sync]
    na, nb = a < _NEAR, b < _NEAR
    with np.errstate(over="ignore"):
        diff = np.where(na != nb, np.where(na, np.int64(I64_MIN), np.int64(I64_MAX)), a - b)
    return dict(counters=counters, type_sync=type_sync, type_status=type_status,
                sync_slot=np.nonzero(t_sync)[0].astype(np.int32), sync_ms=ms(diff).astype(np.int64),
                status_slot=np.nonzero(t_stat)[0].astype(np.int32), status_ms=ms(oos[t_stat]).astype(np.int64),
                n_timers=np.array([t_sync.sum(), t_stat.sum()], np.int32))


@dataclass
class Report:
    """One DoReport: the counters by name, the per-type counts by kind, the timers by meter key (ascending slot)."""
    counts: Dict[str, int] = field(default_factory=dict)          # latency5min.count ... latency1day.status.count
    type_sync: Dict[str, int] = field(default_factory=dict)       # the kinds with a non-zero count only
    type_status: Dict[str, int] = field(default_factory=dict)
    sync_timers: List[Tuple[str, int]] = field(default_factory=list)
    status_timers: List[Tuple[str, int]] = field(default_factory=list)
    sync_throughput: int = 0
    status_throughput: int = 0

    @classmethod
    def from_result(cls, table: MeterTable, r: dict) -> "Report":
        rep = cls()
        for b, (name, _) in enumerate(BUCKETS):
            rep.counts[name + ".count"] = int(r["counters"][b])
            rep.counts[name + ".status.count"] = int(r["counters"][6 + b])
        kinds = table.kind_names
        rep.type_sync = {kinds[i]: int(v) for i, v in enumerate(r["type_sync"][:len(kinds)]) if v}
        rep.type_status = {kinds[i]: int(v) for i, v in enumerate(r["type_status"][:len(kinds)]) if v}
        rep.sync_timers = [(table.key_of[int(s)], int(m)) for s, m in zip(r["sync_slot"], r["sync_ms"])]
        rep.status_timers = [(table.key_of[int(s)], int(m)) for s, m in zip(r["status_slot"], r["status_ms"])]
        rep.sync_throughput, rep.status_throughput = int(r["counters"][12]), int(r["counters"][13])
        return rep

    def to_metrics(self) -> List[tuple]:
        """(op, name, value, tags) in report.go's order of calls: op is ``store`` or ``timer``, tags a tuple of
        (name, value). Where the reference ranges over a Go map or the sync.Map its order is unspecified; here the
        buckets ascend, the kinds follow their interning and the timers ascend by slot."""
        m: List[tuple] = [("store", n + ".count", self.counts[n + ".count"], ()) for n, _ in BUCKETS]
        m += [("store", n + ".status.count", self.counts[n + ".status.count"], ()) for n, _ in BUCKETS]
        m += [("store", "typelatency5min.count", v, (("type", k),)) for k, v in self.type_sync.items()]
        m += [("store", "typelatency5min.status.count", v, (("type", k),)) for k, v in self.type_status.items()]
        m += [("timer", "totalsync.latency.ms", v, (("resourcename", k),)) for k, v in self.sync_timers]
        m.append(("store", "totalsync.throughput", self.sync_throughput, ()))
        m += [("timer", "totalstatus.latency.ms", v, (("resourcename", k),)) for k, v in self.status_timers]
        m.append(("store", "totalstatus.throughput", self.status_throughput, ()))
        return m
