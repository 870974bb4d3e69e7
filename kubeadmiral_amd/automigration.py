"""The auto-migration controller: estimated capacity from unschedulable pods.

``Controller.reconcile`` (pkg/controllers/automigration/controller.go:178-290) runs per federated object
that carries the scheduler's ``pod-unschedulable-threshold`` annotation: for every member-cluster object it
lists the pods (``getPodsFromCluster``, :417-440), counts those that have been unschedulable for longer than the
threshold (``countUnschedulablePods``, util.go:29-64), derives the cluster's estimated capacity
(``estimateCapacity``, :292-378) and writes ``kubeadmiral.io/auto-migration-info`` if the map differs from the
one the object holds (:237-255). The scheduler reads that annotation back into
``AutoMigration.EstimatedCapacity`` (objects.scheduling_unit_for_fed_object) and hashes it into the scheduling
trigger (objects.trigger_prefix).

This module holds the per-object restatement (:func:`estimate_capacity`, :func:`reconcile_object`) and the
batch form: :class:`MigrationBatch` packs objects, (object, cluster) segments and pod records into the arrays of
``kad_migrate_estimate`` (include/kad_sched.h), which counts and compares on the GPU;
:meth:`MigrationBatch.apply` edits the annotation of the objects the device reports as changed.

Listing pods from member clusters is I/O and stays with the caller (automigration/plugins/deployments.go): a
listing arrives as a list of pod dicts, or as an exception object for a listing that failed
(:class:`PodListError` carries ``clusterNeedsBackoff``).

Times are int64 Unix nanoseconds and one ``now_ns`` serves a whole call (the reference calls ``time.Now()`` per
cluster). A pod whose ``lastTransitionTime`` is absent or null holds Go's zero time, which Unix nanoseconds
cannot express: it carries ``POD_TZERO`` and always counts as crossed (``Time.Sub`` saturates to the minimum
duration for any now >= 1970 and any threshold of the domain).
"""

from __future__ import annotations

import calendar
import re
from dataclasses import dataclass
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

from . import gojson as J
from . import objects as O

SEG_SKIP, SEG_BACKOFF = 1, 2                    # KAD_MIG_SEG_*
POD_DELETING, POD_UNSCHED, POD_TZERO = 1, 2, 4  # KAD_MIG_POD_*
TIME_MAX = 1 << 61                              # KAD_MIG_TIME_MAX: |t|, |threshold| and now stay below it
NONE = (1 << 63) - 1                            # next_cross / retry_after: none

POD_SCHEDULED = "PodScheduled"                  # corev1.PodScheduled
CONDITION_FALSE = "False"                       # corev1.ConditionFalse
REASON_UNSCHEDULABLE = "Unschedulable"          # corev1.PodReasonUnschedulable


class PodListError(Exception):
    """getPodsFromCluster failed (controller.go:417-440); ``needs_backoff`` is its clusterNeedsBackoff: true
    when the cluster's client or the listing itself failed, false when the type has no pod plugin."""

    def __init__(self, msg: str = "", needs_backoff: bool = True):
        super().__init__(msg)
        self.needs_backoff = needs_backoff


@dataclass
class _Info:
    ec: Optional[Dict[str, int]] = None


_INFO = J.struct(_Info, [("estimatedCapacity", "ec", J.map_of(J.INT64))])  # framework/types.go:77-80

_RFC3339 = re.compile(r"^(\d{4})-(\d{2})-(\d{2})T(\d{2}):(\d{2}):(\d{2})(?:[.,](\d+))?(Z|[+-]\d{2}:\d{2})$")


def parse_time(s) -> Optional[int]:
    """metav1.Time.UnmarshalJSON (apimachinery meta/v1/time.go): ``null`` is the zero time, otherwise
    ``time.Parse(time.RFC3339, s)``, which also accepts a fractional second (digits past the ninth are dropped).
    Returns Unix nanoseconds, or None for Go's zero time (year 1). ObjectError where Go returns an error."""
    if s is None:
        return None
    if not isinstance(s, str):
        raise O.ObjectError(f"cannot unmarshal {type(s).__name__} into a metav1.Time")
    m = _RFC3339.match(s)
    if not m:
        raise O.ObjectError(f'parsing time "{s}" as RFC 3339')
    y, mo, d, hh, mm, ss = (int(x) for x in m.groups()[:6])
    if not (1 <= mo <= 12 and 1 <= d <= calendar.monthrange(max(y, 1), mo)[1] and hh < 24 and mm < 60 and ss < 60):
        raise O.ObjectError(f'parsing time "{s}": out of range')
    frac = int((m.group(7) or "0")[:9].ljust(9, "0"))
    off = 0
    if m.group(8) != "Z":
        oh, om = int(m.group(8)[1:3]), int(m.group(8)[4:6])
        if oh > 23 or om > 59:
            raise O.ObjectError(f'parsing time "{s}": time zone offset out of range')
        off = (oh * 3600 + om * 60) * (-1 if m.group(8)[0] == "-" else 1)
    # days from the civil date (proleptic Gregorian, as Go's): date.toordinal has no year 0, which Go accepts
    yy = y - (mo <= 2)
    era = yy // 400
    yoe = yy - era * 400
    doy = (153 * (mo + (-3 if mo > 2 else 9)) + 2) // 5 + d - 1
    days = era * 146097 + yoe * 365 + yoe // 4 - yoe // 100 + doy - 719468
    ns = ((days * 86400 + hh * 3600 + mm * 60 + ss - off) * 10**9) + frac
    if ns == -62135596800 * 10**9:  # 0001-01-01T00:00:00Z: time.Time{}
        return None
    return ns


def _conditions(pod: dict) -> list:
    st = pod.get("status") if isinstance(pod, dict) else None
    cs = st.get("conditions") if isinstance(st, dict) else None
    return cs if isinstance(cs, list) else []


def pod_record(pod: dict) -> Tuple[int, int]:
    """One pod as kad_migrate_estimate reads it: (flags, t_ns). util.go:34-61 — a deletion timestamp sets
    POD_DELETING; the FIRST condition of type PodScheduled decides (later ones are ignored, :40-46): POD_UNSCHED
    iff its status is "False" and its reason "Unschedulable"; t_ns is its lastTransitionTime, POD_TZERO (and
    t_ns 0) where that is absent or null. A time that int64 nanoseconds cannot hold is an ObjectError."""
    flags, t = 0, 0
    meta = pod.get("metadata") if isinstance(pod, dict) else None
    if isinstance(meta, dict) and meta.get("deletionTimestamp") is not None:
        flags |= POD_DELETING
    for c in _conditions(pod):
        if isinstance(c, dict) and c.get("type") == POD_SCHEDULED:
            if c.get("status") == CONDITION_FALSE and c.get("reason") == REASON_UNSCHEDULABLE:
                flags |= POD_UNSCHED
                ns = parse_time(c.get("lastTransitionTime"))
                if ns is None:
                    flags |= POD_TZERO
                elif not -(1 << 63) <= ns < (1 << 63):
                    raise O.ObjectError(f"lastTransitionTime {c.get('lastTransitionTime')!r} outside int64 nanoseconds")
                else:
                    t = ns
            break
    return flags, t


def count_unschedulable_pods(pods: Sequence, now_ns: int, threshold_ns: int) -> Tuple[int, Optional[int]]:
    """countUnschedulablePods (util.go:29-64) over pod dicts or (flags, t_ns) records:
    (unschedulableCount, nextCrossIn or None)."""
    count, next_cross = 0, None
    for p in pods:
        flags, t = p if isinstance(p, tuple) else pod_record(p)
        if flags & POD_DELETING or not flags & POD_UNSCHED:
            continue
        crossing = -1 if flags & POD_TZERO else t + threshold_ns - now_ns
        if crossing <= 0:
            count += 1
        elif next_cross is None or next_cross > crossing:
            next_cross = crossing
    return count, next_cross


def total_and_ready_replicas(type_config: O.FederatedTypeConfig, cluster_obj: dict) -> Tuple[int, int]:
    """getTotalAndReadyReplicas (controller.go:380-404): absent values default to 0; ObjectError on a value of
    another type."""
    total = O.get_int64_from_path(cluster_obj, type_config.replicas_status, ())
    ready = O.get_int64_from_path(cluster_obj, type_config.ready_replicas_status, ())
    return total or 0, ready or 0


def desired_replicas(type_config: O.FederatedTypeConfig, cluster_obj: dict) -> int:
    """getDesiredReplicas (controller.go:406-415): ObjectError if absent or of another type."""
    v = O.get_int64_from_path(cluster_obj, type_config.replicas_spec, ())
    if v is None:
        raise O.ObjectError(f"no desired replicas at {type_config.replicas_spec}")
    return v


def segment_of(type_config: O.FederatedTypeConfig, cluster_obj: dict, listing) -> Tuple[int, int]:
    """(flags, desired) of one member-cluster object — what estimateCapacity decides before it counts
    (controller.go:310-330): SEG_SKIP when total == ready with no error, when the desired replicas cannot be
    read, or when the listing failed (SEG_BACKOFF with it if that failure asks for a backoff)."""
    try:
        total, ready = total_and_ready_replicas(type_config, cluster_obj)
        if total == ready:
            return SEG_SKIP, 0
    except O.ObjectError:
        pass  # :311 skips only when err == nil
    try:
        desired = desired_replicas(type_config, cluster_obj)
    except O.ObjectError:
        return SEG_SKIP, 0
    if isinstance(listing, BaseException):
        return SEG_SKIP | (SEG_BACKOFF if getattr(listing, "needs_backoff", False) else 0), desired
    return 0, desired


def cluster_capacity(n_pods: int, desired: int, unschedulable: int) -> Optional[int]:
    """controller.go:345-366: the capacity written for a cluster, None for no entry."""
    cap = n_pods - unschedulable if n_pods >= desired else desired - unschedulable
    if cap >= desired:
        return None
    if cap < 0:  # unreachable for consistent inputs (unschedulable <= n_pods); kept as the reference has it
        cap = 0
    return cap


def estimate_capacity(type_config: O.FederatedTypeConfig, cluster_objs: Sequence[Tuple[str, dict]], pods: Sequence,
                      now_ns: int, threshold_ns: int) -> Tuple[Dict[str, int], Optional[Tuple[Optional[int], bool]]]:
    """estimateCapacity (controller.go:292-378) for one object: ``cluster_objs`` are (cluster name, member
    object) pairs, ``pods[j]`` the pod dicts (or records) of pair j or an exception. Returns (estimatedCapacity,
    result) with result None or (retry_after_ns or None, backoff) — worker.Result's RequeueAfter and Backoff."""
    caps: Dict[str, int] = {}
    backoff, retry = False, None
    for (name, cobj), listing in zip(cluster_objs, pods):
        flags, desired = segment_of(type_config, cobj, listing)
        if flags & SEG_BACKOFF:
            backoff = True
        if flags & SEG_SKIP:
            continue
        uns, nxt = count_unschedulable_pods(listing, now_ns, threshold_ns)
        if nxt is not None and (retry is None or nxt < retry):
            retry = nxt
        cap = cluster_capacity(len(listing), desired, uns)
        if cap is not None:
            caps[name] = cap
    return caps, ((retry, backoff) if backoff or retry is not None else None)


def marshal_info(caps: Optional[Dict[str, int]]) -> str:
    """json.Marshal(&AutoMigrationInfo{EstimatedCapacity: caps}) (framework/types.go:77-80): map keys sorted
    (by their UTF-8 bytes, as Go sorts strings), ``{}`` for a nil or empty map (omitempty)."""
    if not caps:
        return "{}"
    keys = sorted(caps, key=lambda k: k.encode("utf-8", "surrogatepass"))
    return '{"estimatedCapacity":{' + ",".join(J.encode_string(k) + ":" + str(int(caps[k])) for k in keys) + "}}"


def decode_info(text: Optional[str]) -> Optional[Dict[str, int]]:
    """The existing annotation as reconcile reads it (controller.go:238-245): None for an absent annotation, a
    null / absent map, or text that does not unmarshal (treated as if it did not exist)."""
    if text is None:
        return None
    try:
        return J.unmarshal(text, _INFO).ec
    except J.GoJSONError:
        return None


def info_changed(existing: Optional[Dict[str, int]], new: Optional[Dict[str, int]]) -> bool:
    """!equality.Semantic.DeepEqual of two AutoMigrationInfo (controller.go:247): nil and empty maps are equal."""
    return (existing or {}) != (new or {})


def threshold_of(obj: dict) -> Optional[int]:
    """The scheduler's pod-unschedulable-threshold annotation as nanoseconds; None when it is absent or does
    not parse (controller.go:200-209): auto migration is disabled for the object."""
    v = (O.get_annotations(obj) or {}).get(O.POD_UNSCHEDULABLE_THRESHOLD_ANNOTATION)
    if v is None:
        return None
    try:
        return O.parse_duration(v)
    except O.ObjectError:
        return None


def apply(obj: dict, caps: Optional[Dict[str, int]], enabled: bool = True, changed: Optional[bool] = None) -> bool:
    """The annotation edit of reconcile (controller.go:217-224, 247-261), in place; returns needsUpdate.
    Disabled: the info annotation is deleted if present. Enabled: it is set to :func:`marshal_info` of ``caps``
    when the maps differ (``changed``: that comparison's outcome where the caller already has it)."""
    ann = O.get_annotations(obj) or {}
    if not enabled:
        if O.AUTO_MIGRATION_INFO_ANNOTATION not in ann:
            return False
        del ann[O.AUTO_MIGRATION_INFO_ANNOTATION]
        O.set_annotations(obj, ann)
        return True
    if changed is None:
        changed = info_changed(decode_info(ann.get(O.AUTO_MIGRATION_INFO_ANNOTATION)), caps)
    if not changed:
        return False
    ann[O.AUTO_MIGRATION_INFO_ANNOTATION] = marshal_info(caps)
    O.set_annotations(obj, ann)
    return True


def reconcile_object(type_config: O.FederatedTypeConfig, obj: dict, cluster_objs, pods, now_ns: int):
    """Controller.reconcile for one object on the host (the per-object path the batch is checked against):
    (result, estimatedCapacity or None when disabled, needsUpdate); ``obj`` is edited in place."""
    thr = threshold_of(obj)
    if thr is None:
        return None, None, apply(obj, None, enabled=False)
    caps, result = estimate_capacity(type_config, cluster_objs, pods, now_ns, thr)
    return result, caps, apply(obj, caps)


class MigrationBatch:
    """The arrays of one kad_migrate_estimate: objects with a threshold, their segments sorted by cluster id
    (the snapshot's ids first, other names interned after them), the pod records, and the existing annotations
    as a sorted CSR. ``snapshot_names``: the resident snapshot's cluster names in id order."""

    def __init__(self, type_config: O.FederatedTypeConfig, snapshot_names: Sequence[str], now_ns: int):
        self.type_config = type_config
        self.C = len(snapshot_names)
        self.names: List[str] = list(snapshot_names)
        self.at: Dict[str, int] = {n: i for i, n in enumerate(self.names)}
        self.now_ns = int(now_ns)
        self.thr: List[int] = []
        self.seg_off: List[int] = [0]
        self.seg_cluster: List[int] = []
        self.seg_desired: List[int] = []
        self.seg_flags: List[int] = []
        self.pod_off: List[int] = [0]
        self.pod_t: List[int] = []
        self.pod_flags: List[int] = []
        self.old_off: List[int] = [0]
        self.old_cluster: List[int] = []
        self.old_cap: List[int] = []

    def intern(self, name: str) -> int:
        i = self.at.get(name)
        if i is None:
            i = self.at[name] = len(self.names)
            self.names.append(name)
        return i

    def add(self, obj: dict, threshold_ns: int, cluster_objs: Sequence[Tuple[str, dict]], pods: Sequence) -> int:
        """One enabled object; returns its index in the batch. A cluster appears once (GetFromAllClusters
        returns one object per member cluster): a repeated name is a ValueError."""
        segs = sorted((self.intern(name), j) for j, (name, _) in enumerate(cluster_objs))
        if any(a[0] == b[0] for a, b in zip(segs, segs[1:])):
            raise ValueError("a cluster name occurs twice among an object's member-cluster objects")
        for cid, j in segs:
            flags, desired = segment_of(self.type_config, cluster_objs[j][1], pods[j])
            self.seg_cluster.append(cid)
            self.seg_desired.append(desired)
            self.seg_flags.append(flags)
            if not flags & SEG_SKIP:
                for p in pods[j]:
                    f, t = p if isinstance(p, tuple) else pod_record(p)
                    self.pod_flags.append(f)
                    self.pod_t.append(t)
            self.pod_off.append(len(self.pod_t))
        self.seg_off.append(len(self.seg_cluster))
        old = decode_info((O.get_annotations(obj) or {}).get(O.AUTO_MIGRATION_INFO_ANNOTATION)) or {}
        for cid, cap in sorted((self.intern(k), v) for k, v in old.items()):
            self.old_cluster.append(cid)
            self.old_cap.append(cap)
        self.old_off.append(len(self.old_cluster))
        self.thr.append(int(threshold_ns))
        return len(self.thr) - 1

    def arrays(self) -> dict:
        """The keyword arguments of runtime.migrate_args / Context.migrate_estimate."""
        return dict(n_ids=len(self.names), now_ns=self.now_ns,
                    obj_seg_off=np.array(self.seg_off, np.int32), obj_threshold_ns=np.array(self.thr, np.int64),
                    seg_cluster=np.array(self.seg_cluster, np.int32), seg_desired=np.array(self.seg_desired, np.int64),
                    seg_flags=np.array(self.seg_flags, np.uint8), seg_pod_off=np.array(self.pod_off, np.int64),
                    pod_t_ns=np.array(self.pod_t, np.int64), pod_flags=np.array(self.pod_flags, np.uint8),
                    old_off=np.array(self.old_off, np.int32), old_cluster=np.array(self.old_cluster, np.int32),
                    old_cap=np.array(self.old_cap, np.int64))

    def capacities(self, r: dict, i: int) -> Dict[str, int]:
        """Object i's estimatedCapacity from kad_migrate_estimate's outputs."""
        s0, s1 = self.seg_off[i], self.seg_off[i + 1]
        cap = r["cap"]
        return {self.names[self.seg_cluster[s]]: int(cap[s]) for s in range(s0, s1) if cap[s] >= 0}

    @staticmethod
    def result(r: dict, i: int) -> Optional[Tuple[Optional[int], bool]]:
        """Object i's worker result (controller.go:369-377): None, or (retry_after_ns or None, backoff)."""
        retry, backoff = int(r["retry_after"][i]), bool(r["backoff"][i])
        if retry == NONE and not backoff:
            return None
        return (None if retry == NONE else retry), backoff

    def apply(self, objs: Sequence[dict], r: dict) -> List[bool]:
        """The annotation edit for the batch's objects (``objs[i]`` = the object of index i), in place: only the
        objects the device reports as changed are touched. Returns needsUpdate per object."""
        out = []
        for i, obj in enumerate(objs):
            out.append(bool(r["changed"][i]) and apply(obj, self.capacities(r, i), changed=True))
        return out


def _seg_reduce(ufunc, a: np.ndarray, off: np.ndarray, empty) -> np.ndarray:
    """ufunc.reduceat over the CSR rows of ``a``; ``empty`` for rows without elements (which reduceat cannot
    express: it is called on the starts of the non-empty rows only)."""
    lens = off[1:] - off[:-1]
    out = np.full(len(lens), empty, a.dtype)
    ne = lens > 0
    if ne.any():
        out[ne] = ufunc.reduceat(a, off[:-1][ne])
    return out


def migrate_numpy(n_ids: int, now_ns: int, **a) -> dict:
    """kad_migrate_estimate restated with numpy on one thread (np.add.reduceat / np.minimum.reduceat over the
    same arrays): what the cost script compares the device with, and what synth.gen_migration derives
    existing annotations from. Inputs are assumed valid."""
    so, po = a["obj_seg_off"].astype(np.int64), a["seg_pod_off"]
    S, Oc = len(a["seg_cluster"]), len(a["obj_threshold_ns"])
    seg_obj = np.repeat(np.arange(Oc), so[1:] - so[:-1])
    skip = (a["seg_flags"] & SEG_SKIP) != 0
    n = np.where(skip, 0, po[1:] - po[:-1])
    pod_seg = np.repeat(np.arange(S), po[1:] - po[:-1])
    f = a["pod_flags"]
    live = ((f & (POD_DELETING | POD_UNSCHED)) == POD_UNSCHED) & ~skip[pod_seg]
    crossing = a["pod_t_ns"] + a["obj_threshold_ns"][seg_obj][pod_seg] - now_ns
    crossed = live & (((f & POD_TZERO) != 0) | (crossing <= 0))
    uns = _seg_reduce(np.add, crossed.astype(np.int64), po, 0)
    nxt = _seg_reduce(np.minimum, np.where(live & ~crossed, crossing, NONE), po, NONE)
    desired = a["seg_desired"]
    cap = np.where(n >= desired, n - uns, desired - uns)
    cap = np.where(skip | (cap >= desired), -1, np.maximum(cap, 0))
    written = cap >= 0
    n_written = _seg_reduce(np.add, written.astype(np.int64), so, 0)
    retry = _seg_reduce(np.minimum, nxt, so, NONE)
    backoff = _seg_reduce(np.maximum, ((a["seg_flags"] & SEG_BACKOFF) != 0).astype(np.int64), so, 0)
    oo = a["old_off"].astype(np.int64)
    n_old = oo[1:] - oo[:-1]
    changed = n_written != n_old
    wcl, wcap, wobj = a["seg_cluster"][written], cap[written], seg_obj[written]
    woff = np.zeros(Oc + 1, np.int64)
    woff[1:] = np.cumsum(n_written)
    same = ~changed[wobj]  # entry k of an object with as many old entries stands against old entry k
    k = np.arange(len(wcl)) - woff[wobj]
    at = (oo[wobj] + k)[same]
    diff = (a["old_cluster"][at] != wcl[same]) | (a["old_cap"][at] != wcap[same])
    changed = changed.copy()
    np.logical_or.at(changed, wobj[same][diff], True)
    return {"uns": uns.astype(np.int32), "next_cross": nxt, "cap": cap, "changed": changed.astype(np.uint8),
            "n_written": n_written.astype(np.int32), "retry_after": retry, "backoff": backoff.astype(np.uint8)}
