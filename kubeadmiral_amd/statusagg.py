"""Status aggregation: the source object's status from its member clusters' copies.

The reference's status aggregator (pkg/controllers/statusaggregator/controller.go:249-348) runs, per source object
and on every member-object event, ``IsResourcePropagated`` and a plugin's ``AggregateStatuses``. This module
restates both per object in the reference's structure (:func:`is_resource_propagated`,
:func:`aggregate_deployment`, :func:`aggregate_job`, :func:`latest_replicaset_digest`), packs a batch of objects of
one kind into kad_status_aggregate's columns (:class:`StatusAggBatch`), writes the device's results back
(:meth:`StatusAggBatch.apply`) and restates the device call with numpy (:func:`sagg_numpy`).

Objects are unstructured dicts. A Python ``int`` stands for Go's int64 and a ``float`` for float64 (bool is
neither); ``None`` as a member's ``status`` stands for the nil map the plugins skip. Times are RFC 3339 strings,
held as Unix seconds: whole seconds are the resolution of metav1.Time's JSON form.
"""

from __future__ import annotations

import calendar
import copy
import datetime
import json
import math
import re
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

from . import gojson

DEPLOYMENT, JOB = 0, 1  # KAD_SAGG_DEPLOYMENT / KAD_SAGG_JOB
OBJ_UPTODATE, OBJ_ERROR, OBJ_OLD_OTHER = 1, 2, 4
SEG_NIL, SEG_SYNCED, SEG_START, SEG_DONE, SEG_FAILED = 1, 2, 4, 8, 16
TIME_MAX = 1 << 61
TIME_ZERO = -62135596800  # time.Time{} as Unix seconds (year 1): IsZero
NO_START, NO_DONE = np.iinfo(np.int64).max, np.iinfo(np.int64).min
DEP_FIELDS = ("replicas", "updatedReplicas", "readyReplicas", "availableReplicas", "unavailableReplicas")
JOB_FIELDS = ("active", "succeeded", "failed")
I32_MIN, I32_MAX, I64_MIN, I64_MAX = -(1 << 31), (1 << 31) - 1, -(1 << 63), (1 << 63) - 1

PREFIX = "kubeadmiral.io/"
FEDERATE_PREFIX = "federate.controller." + PREFIX
OBSERVED_ANNOTATION_KEYS = FEDERATE_PREFIX + "observed-annotations"
OBSERVED_LABEL_KEYS = FEDERATE_PREFIX + "observed-labels"
TEMPLATE_MERGE_PATCH = FEDERATE_PREFIX + "template-generator-merge-patch"
SOURCE_GENERATION = PREFIX + "source-generation"
RS_NAME = "latestreplicaset.kubeadmiral.io/name"
RS_REPLICAS = "latestreplicaset.kubeadmiral.io/replicas"
RS_AVAILABLE = "latestreplicaset.kubeadmiral.io/available-replicas"
RS_READY = "latestreplicaset.kubeadmiral.io/ready-replicas"
RS_OBSERVED_GENERATION = "latestreplicaset.kubeadmiral.io/observed-generation"
RS_DIGESTS = PREFIX + "latest-replicaset-digests"

# objects the batch answers with the per-object path: the device's time domain has no place for them
HOST_ZERO_TIME = "a set time that IsZero: the reference's start-time rule depends on its map order (parity unpinned)"
HOST_SUBSECOND = "a time with a fraction of a second"


class StatusAggError(Exception):
    """An error return of the reference: the object's worker status is StatusError."""


# ------------------------------------------------------------------ unstructured helpers
def _is_int(v) -> bool:
    return isinstance(v, int) and not isinstance(v, bool)


def _whole(v) -> bool:
    """A float64 that json.Marshal writes as an integer literal."""
    return isinstance(v, float) and math.isfinite(v) and v == int(v)


def deep_equal(a, b) -> bool:
    """reflect.DeepEqual of two unstructured values: the dynamic types must match (int64 1 != float64 1)."""
    if isinstance(a, dict) or isinstance(b, dict):
        return (isinstance(a, dict) and isinstance(b, dict) and a.keys() == b.keys()
                and all(deep_equal(v, b[k]) for k, v in a.items()))
    if isinstance(a, list) or isinstance(b, list):
        return (isinstance(a, list) and isinstance(b, list) and len(a) == len(b)
                and all(deep_equal(x, y) for x, y in zip(a, b)))
    return type(a) is type(b) and a == b


def _nested(obj, *path):
    """unstructured.NestedFieldNoCopy → (value, found); StatusAggError where a parent is not a map."""
    v = obj
    for p in path:
        if v is None:
            return None, False
        if not isinstance(v, dict):
            raise StatusAggError(f"{'.'.join(path)}: accessor error")
        if p not in v:
            return None, False
        v = v[p]
    return v, True


def _string_map(obj, *path) -> Dict[str, str]:
    """GetAnnotations / GetLabels (NestedStringMap, errors dropped)."""
    try:
        m, found = _nested(obj, *path)
    except StatusAggError:
        return {}
    if not found or not isinstance(m, dict) or not all(isinstance(v, str) for v in m.values()):
        return {}
    return m


def _generation(obj) -> int:
    try:
        g, found = _nested(obj, "metadata", "generation")
    except StatusAggError:
        return 0
    return g if found and _is_int(g) else 0


_RFC3339 = re.compile(r"^(\d{4})-(\d\d)-(\d\d)[Tt](\d\d):(\d\d):(\d\d)(\.\d+)?([Zz]|[+-]\d\d:\d\d)$")


def parse_time(v) -> Optional[Tuple[int, int]]:
    """metav1.Time.UnmarshalJSON: None for null, else (Unix seconds, nanoseconds) of an RFC 3339 string."""
    if v is None:
        return None
    m = _RFC3339.match(v) if isinstance(v, str) else None
    if not m:
        raise StatusAggError(f"cannot parse {v!r} as a time")
    y, mo, d, h, mi, s = (int(m.group(i)) for i in range(1, 7))
    try:
        sec = calendar.timegm(datetime.datetime(y, mo, d, h, mi, s).timetuple()) if y >= 1 else None
    except ValueError:
        sec = None
    if sec is None:
        raise StatusAggError(f"cannot parse {v!r} as a time")
    z = m.group(8)
    if z not in "Zz":
        sec -= (1 if z[0] == "+" else -1) * (int(z[1:3]) * 3600 + int(z[4:6]) * 60)
    return sec, int(((m.group(7) or ".0")[1:] + "0" * 9)[:9])


def format_time(sec: int) -> Optional[str]:
    """metav1.Time.MarshalJSON: UTC, whole seconds; null for the zero time."""
    if sec == TIME_ZERO:
        return None
    return (datetime.datetime(1970, 1, 1) + datetime.timedelta(seconds=int(sec))).strftime("%Y-%m-%dT%H:%M:%SZ")


def _is_zero(t: Optional[Tuple[int, int]]) -> bool:
    return t is None or t == (TIME_ZERO, 0)


# ------------------------------------------------------------------ IsResourcePropagated
def _merge_patch(doc, patch):
    """RFC 7386, as evanphx/json-patch MergePatch applies it to decoded documents."""
    if not isinstance(patch, dict):
        return copy.deepcopy(patch)
    out = dict(doc) if isinstance(doc, dict) else {}
    for k, v in patch.items():
        if v is None:
            out.pop(k, None)
        else:
            out[k] = _merge_patch(out.get(k), v)
    return out


def _as_decoded(v):
    """A value after json.Marshal and the client-go style decoding: integral floats come back as int64."""
    if isinstance(v, dict):
        return {k: _as_decoded(x) for k, x in v.items()}
    if isinstance(v, list):
        return [_as_decoded(x) for x in v]
    if _whole(v) and abs(v) < 1e21:
        return int(v)
    return v


def _observed_keys(keys: str):
    seg = keys.split("|")
    if len(seg) != 2:
        return set(), set()
    return (set(seg[0].split(",")) if seg[0] else set()), (set(seg[1].split(",")) if seg[1] else set())


def _maps_synced(src: Dict[str, str], fed: Dict[str, str], observed: str) -> bool:
    fed_keys, ignored = _observed_keys(observed)
    if (fed_keys | ignored) != set(src):
        return False
    return all(src.get(k, "") == fed.get(k, "") for k in fed_keys)


def is_federated_template_up_to_date(source: dict, fed: dict) -> bool:
    """IsFederatedTemplateUpToDate (util/propagationstatus/propagationstatus.go:88-128)."""
    template, found = _nested(fed, "spec", "template")
    if not found:
        return False
    if not isinstance(template, dict):
        raise StatusAggError("spec.template: accessor error")
    ann = _string_map(fed, "metadata", "annotations")
    if not ann:
        return False
    if not _maps_synced(_string_map(source, "metadata", "annotations"), ann, ann.get(OBSERVED_ANNOTATION_KEYS, "")):
        return False
    if not _maps_synced(_string_map(source, "metadata", "labels"), _string_map(fed, "metadata", "labels"),
                        ann.get(OBSERVED_LABEL_KEYS, "")):
        return False
    try:
        patch = json.loads(ann.get(TEMPLATE_MERGE_PATCH, ""))
    except Exception as e:  # noqa: BLE001 - an invalid merge patch is the reference's error return
        raise StatusAggError(f"invalid merge patch: {e}") from None
    return deep_equal(_merge_patch(_as_decoded(source), patch), template)


def is_resource_propagated(source: Optional[dict], fed: Optional[dict]) -> bool:
    """propagationstatus.IsResourcePropagated (propagationstatus.go:34-72): clusterObjsUpToDate."""
    if source is None:
        raise StatusAggError("source object can't be nil")
    if fed is None:
        return False
    if not is_federated_template_up_to_date(source, fed):
        return False
    synced, found = _nested(fed, "status", "syncedGeneration")
    if not found:
        return False
    if not _is_int(synced):
        raise StatusAggError("status.syncedGeneration: accessor error")
    if synced != _generation(fed):
        return False
    status = fed.get("status")
    if status is None:
        return False
    return all(_dict(c).get("status", "") == "OK" for c in _list(status.get("clusters")))


def _dict(v) -> dict:
    return v if isinstance(v, dict) else {}


def _list(v) -> list:
    return v if isinstance(v, list) else []


def _synced_generations(fed: Optional[dict]) -> Dict[str, int]:
    """fedObject.status.clusters as name → generation (deployment.go:71-76)."""
    out = {}
    for c in _list(_dict(_dict(fed).get("status")).get("clusters")):
        c = _dict(c)
        g = c.get("generation", 0)
        out[c.get("name", "") if isinstance(c.get("name", ""), str) else ""] = g if _is_int(g) else 0
    return out


# ------------------------------------------------------------------ member statuses
def _member_status(obj) -> Optional[dict]:
    """unstructured.NestedMap(utd.Object, "status"): None for the nil map."""
    if not isinstance(obj, dict) or "status" not in obj:
        raise StatusAggError("status of the cluster object not found")
    s = obj["status"]
    if s is not None and not isinstance(s, dict):
        raise StatusAggError("status of the cluster object is not a map")
    return s


def _json_int(v, lo: int, hi: int, what: str) -> int:
    """A value through json.Marshal / json.Unmarshal into an integer field: null leaves 0; a number must be
    written without fraction or exponent and lie in range."""
    if v is None:
        return 0
    if _whole(v) and abs(v) < 1e21:
        v = int(v)
    if not _is_int(v) or not lo <= v <= hi:
        raise StatusAggError(f"cannot unmarshal {v!r} into {what}")
    return v


def _wrap32(v: int) -> int:
    return (v + (1 << 31)) % (1 << 32) - (1 << 31)


def _converter_int32(v, what: str) -> int:
    """runtime.DefaultUnstructuredConverter into an int32 field: int64 is set without a range check (it wraps),
    float64 must be whole, nil leaves 0, anything else does not convert."""
    if v is None:
        return 0
    if _whole(v) and abs(v) < 2 ** 63:
        v = int(v)
    if not _is_int(v):
        raise StatusAggError(f"cannot convert {v!r} to {what}")
    return _wrap32(v)


def _conditions(v, what: str) -> List[dict]:
    if v is None:
        return []
    if not isinstance(v, list) or not all(isinstance(c, dict) for c in v):
        raise StatusAggError(f"cannot convert {what}")
    for c in v:
        for k in ("type", "status"):
            if not isinstance(c.get(k, ""), str) and c.get(k) is not None:
                raise StatusAggError(f"cannot convert {what}.{k}")
    return v


def deployment_member(status: dict) -> Tuple[List[int], int]:
    """ConvertViaJson(status, &DeploymentStatus) (deployment.go:94-97) → the five counts, observedGeneration."""
    vals = [_json_int(status.get(k), I32_MIN, I32_MAX, "int32") for k in DEP_FIELDS]
    _json_int(status.get("collisionCount"), I32_MIN, I32_MAX, "int32")
    _conditions(status.get("conditions"), "conditions")
    return vals, _json_int(status.get("observedGeneration"), I64_MIN, I64_MAX, "int64")


def job_member(status: dict):
    """FromUnstructured(status, &JobStatus) (job.go:72-76) → the three counts, startTime, completionTime (None or
    (seconds, nanoseconds)) and IsJobFinishedWithFailed."""
    vals = [_converter_int32(status.get(k), "int32") for k in JOB_FIELDS]
    start, done = parse_time(status.get("startTime")), parse_time(status.get("completionTime"))
    failed = any(c.get("type") == "Failed" and c.get("status") == "True" for c in _conditions(status.get("conditions"), "conditions"))
    return vals, start, done, failed


def _old_status(source: dict):
    """unstructured.NestedMap(sourceObject.Object, "status") → the old map, None where it is absent."""
    s, found = _nested(source, "status")
    if found and not isinstance(s, dict):
        raise StatusAggError("status of the source object is not a map")
    return s if found else None


# ------------------------------------------------------------------ Deployment
def latest_replicaset_digest(cluster: str, obj: dict) -> Tuple[dict, List[str]]:
    """util.LatestReplicasetDigestFromObject (util/federatedstatus.go:80-130) → (digest, errors)."""
    errs: List[str] = []
    ann = _string_map(obj, "metadata", "annotations")

    def string_entry(key):
        if key in ann:
            return ann[key], True
        errs.append(f"annotation {key} does not exist")
        return "", False

    def int_entry(key):
        s, ok = string_entry(key)
        if not ok:
            return 0
        i = gojson.atoi(s)
        if i is None:
            errs.append(f"annotation {key} is invalid")
            return 0
        return i

    name, _ = string_entry(RS_NAME)
    digest = {"clusterName": cluster, "replicasetName": name, "replicas": int_entry(RS_REPLICAS),
              "availableReplicas": int_entry(RS_AVAILABLE), "readyReplicas": int_entry(RS_READY)}
    source_generation = int_entry(SOURCE_GENERATION)
    try:
        og, found = _nested(obj, "status", "observedGeneration")
    except StatusAggError:
        og, found = None, False
    if not found or not _is_int(og):
        errs.append("failed to get observedGeneration of cluster resource object")
        og = 0
    digest["observedGeneration"] = og
    digest["sourceGeneration"] = source_generation
    return digest, errs


def digests_annotation(cluster_objs: Dict[str, dict]) -> str:
    """The latest-replicaset digests of the eligible members, sorted by cluster, as json.Marshal writes them
    (deployment.go:112-125, 155-164)."""
    out = []
    for name in sorted(cluster_objs):
        obj = cluster_objs[name]
        if obj.get("status") is None:
            continue  # the loop `continue`s before the digest (deployment.go:89-92)
        if str(_generation(obj)) != _string_map(obj, "metadata", "annotations").get(RS_OBSERVED_GENERATION, ""):
            continue
        digest, errs = latest_replicaset_digest(name, obj)
        if errs:
            continue
        parts = []
        for k, v in digest.items():  # every field is omitempty
            if v:
                parts.append(f"{gojson.encode_string(k)}:{gojson.encode_string(v) if isinstance(v, str) else v}")
        out.append("{" + ",".join(parts) + "}")
    return "[" + ",".join(out) + "]"


def _write_digests(source: dict, cluster_objs: Dict[str, dict]) -> bool:
    """deployment.go:155-185: True if the annotation had to be written."""
    text = digests_annotation(cluster_objs)
    meta = source.setdefault("metadata", {})
    if _string_map(source, "metadata", "annotations").get(RS_DIGESTS) == text:
        return False
    if not isinstance(meta.get("annotations"), dict):
        meta["annotations"] = {}
    meta["annotations"][RS_DIGESTS] = text
    return True


def deployment_status(sums: Sequence[int], observed: int) -> dict:
    """GetUnstructuredStatus(aggregatedStatus): zero fields are omitted; encoding/json decodes the numbers into a
    map as float64 (util/meta.go:159-176)."""
    out = {k: float(v) for k, v in zip(DEP_FIELDS, sums) if v}
    if observed:
        out["observedGeneration"] = float(observed)
    return out


def aggregate_deployment(source: dict, fed: Optional[dict], cluster_objs: Dict[str, dict], up_to_date: bool) -> bool:
    """DeploymentPlugin.AggregateStatuses (plugins/deployment.go:42-186): writes ``source`` in place, returns
    needUpdate; StatusAggError for the reference's error returns (``source`` is then untouched)."""
    generation, observed_old = _source_deployment(source)
    need_generation = bool(up_to_date)
    synced = _synced_generations(fed)
    sums = [0] * 5
    for name, obj in cluster_objs.items():
        status = _member_status(obj)
        if status is None:
            need_generation = False
            continue
        vals, observed = deployment_member(status)
        if name not in synced or synced[name] != observed:
            need_generation = False
        sums = [_wrap32(a + b) for a, b in zip(sums, vals)]
    new = deployment_status(sums, generation if need_generation else observed_old)
    old = _old_status(source)
    need = False
    if not deep_equal(new, old):
        source["status"] = new
        need = True
    return _write_digests(source, cluster_objs) or need


def _source_deployment(source: dict) -> Tuple[int, int]:
    """ConvertViaJson(sourceObject, &Deployment) (deployment.go:53-56), as far as the plugin reads it:
    metadata.generation and status.observedGeneration."""
    meta, status = source.get("metadata"), source.get("status")
    for m in (meta, status):
        if m is not None and not isinstance(m, dict):
            raise StatusAggError("cannot unmarshal the source object into a Deployment")
    g = _json_int(_dict(meta).get("generation"), I64_MIN, I64_MAX, "int64")
    st = _dict(status)
    for k in DEP_FIELDS:
        _json_int(st.get(k), I32_MIN, I32_MAX, "int32")
    return g, _json_int(st.get("observedGeneration"), I64_MIN, I64_MAX, "int64")


# ------------------------------------------------------------------ Job
def job_condition(completed: List[str], failed: List[str], now: int) -> dict:
    """The aggregated condition (job.go:96-128), as ToUnstructured writes it."""
    completed, failed = sorted(completed), sorted(failed)
    if completed and failed:
        typ, reason = "Failed", "Mixed"
        msg = f"Job completed in clusters [{','.join(completed)}] and failed in member clusters [{','.join(failed)}]"
    elif completed:
        typ, reason, msg = "Complete", "Completed", f"Job completed in clusters [{','.join(completed)}]"
    else:
        typ, reason, msg = "Failed", "Failed", f"Job failed in clusters [{','.join(failed)}]"
    t = format_time(now)
    return {"type": typ, "status": "True", "lastProbeTime": t, "lastTransitionTime": t, "reason": reason, "message": msg}


def job_status(sums: Sequence[int], start: Optional[int], done: Optional[int], condition: Optional[dict]) -> dict:
    """ToUnstructured(aggregatedStatus): nil pointers and zero counts are omitted, counts are int64."""
    out: dict = {}
    if condition is not None:
        out["conditions"] = [condition]
    if start is not None:
        out["startTime"] = format_time(start)
    if done is not None:
        out["completionTime"] = format_time(done)
    out.update({k: int(v) for k, v in zip(JOB_FIELDS, sums) if v})
    return out


def aggregate_job(source: dict, fed: Optional[dict], cluster_objs: Dict[str, dict], up_to_date: bool, now: int) -> bool:
    """JobPlugin.AggregateStatuses (plugins/job.go:43-153) over the members in the given (Go: map) order: writes
    ``source`` in place, returns needUpdate. ``now`` (Unix seconds) stamps the aggregated condition."""
    sums = [0] * 3
    start: Optional[Tuple[int, int]] = None
    completion: Optional[Tuple[int, int]] = None
    completed, failed = [], []
    for name, obj in cluster_objs.items():
        status = _member_status(obj)
        if status is None:
            continue
        vals, st, done, is_failed = job_member(status)
        # Before() is false when either side is nil
        if _is_zero(start) or (st is not None and start is not None and st < start):
            start = st
        if not _is_zero(done):
            completed.append(name)
            if _is_zero(completion) or completion < done:
                completion = done
        elif is_failed:
            failed.append(name)
        sums = [_wrap32(a + b) for a, b in zip(sums, vals)]
    finished = len(completed) + len(failed)
    cond = job_condition(completed, failed, now) if finished > 0 and finished == len(cluster_objs) else None
    all_done = cond is not None and not failed
    new = job_status(sums, None if start is None else start[0], completion[0] if all_done else None, cond)
    old = _old_status(source)
    if deep_equal(new, old):
        return False
    source["status"] = new
    return True


# ------------------------------------------------------------------ the batch
def _old_columns(kind: int, old) -> Tuple[List[int], bool]:
    """The old status as kad_status_aggregate's int64 columns, and whether it can compare equal at all: it
    cannot where the status is absent or holds a key the new status never has, a zero the new one would omit, or
    a value of another dynamic type than the new status' (float64 for a Deployment — GetUnstructuredStatus
    decodes with encoding/json —, int64 and the canonical time text for a Job)."""
    if kind == DEPLOYMENT:
        cols, fields = [0] * 6, DEP_FIELDS + ("observedGeneration",)
    else:
        cols, fields = [0, 0, 0, int(NO_START), int(NO_DONE)], JOB_FIELDS + ("startTime", "completionTime")
    if old is None:
        return cols, False
    ok = True
    for k, v in old.items():
        if k == "conditions" and kind == JOB:
            continue  # compared on the host, with the aggregated condition
        if k not in fields:
            ok = False
        elif k in ("startTime", "completionTime"):
            try:
                t = parse_time(v)
            except StatusAggError:
                t = None
            if t is None or t[1] or not -TIME_MAX <= t[0] <= TIME_MAX or format_time(t[0]) != v:
                ok = False
            else:
                cols[fields.index(k)] = t[0]
        elif kind == DEPLOYMENT:
            if _whole(v) and v != 0 and I64_MIN <= int(v) <= I64_MAX and float(int(v)) == v:
                cols[fields.index(k)] = int(v)
            else:
                ok = False
        elif _is_int(v) and v != 0 and I64_MIN <= v <= I64_MAX:
            cols[fields.index(k)] = v
        else:
            ok = False
    return cols, ok


class StatusAggBatch:
    """A batch of source objects of one kind for kad_status_aggregate.

    ``add`` takes a source object, its federated object and its member objects (cluster name → object) and does
    what needs strings: IsResourcePropagated, the conversion of every member's status, the join with
    ``fedObject.status.clusters``, the old status' columns. ``errors`` holds the objects with an object-level
    error (they ride along flagged ERROR), ``host`` the objects the per-object path answers (with the reason);
    ``device`` lists the others, in the order of the arrays."""

    def __init__(self, kind: int):
        self.kind = kind
        self.raw: List[Tuple[dict, Optional[dict], Dict[str, dict]]] = []
        self.recs: List[Optional[tuple]] = []  # (flags, generation, observed, old columns, segments)
        self.errors: Dict[int, StatusAggError] = {}
        self.host: Dict[int, str] = {}
        self.up_to_date: List[bool] = []
        self.device: List[int] = []

    def add(self, source: dict, fed: Optional[dict], cluster_objs: Dict[str, dict]) -> int:
        i = len(self.raw)
        self.raw.append((source, fed, cluster_objs))
        self.up_to_date.append(False)
        try:
            self.recs.append(self._record(i, source, fed, cluster_objs))
        except StatusAggError as e:
            self.errors[i] = e
            self.recs.append((OBJ_ERROR, 0, 0, _old_columns(self.kind, None)[0], [(0, [0] * (5 if self.kind == DEPLOYMENT else 3), 0, 0)
                                                                                  for _ in cluster_objs]))
        return i

    def _record(self, i: int, source: dict, fed, cluster_objs):
        utd = is_resource_propagated(source, fed)
        self.up_to_date[i] = utd
        flags = OBJ_UPTODATE if utd else 0
        generation = observed = 0
        if self.kind == DEPLOYMENT:
            generation, observed = _source_deployment(source)
            synced = _synced_generations(fed)
        segs = []
        for name, obj in cluster_objs.items():
            status = _member_status(obj)
            if status is None:
                segs.append((SEG_NIL, [0] * (5 if self.kind == DEPLOYMENT else 3), 0, 0))
            elif self.kind == DEPLOYMENT:
                vals, og = deployment_member(status)
                segs.append((SEG_SYNCED if name in synced else 0, vals, og, synced.get(name, 0)))
            else:
                vals, st, done, failed = job_member(status)
                if (st is not None and st[1]) or (done is not None and done[1]):
                    self.host[i] = HOST_SUBSECOND
                if st == (TIME_ZERO, 0):
                    self.host[i] = HOST_ZERO_TIME
                f = SEG_START if st is not None else 0
                if not _is_zero(done):
                    f |= SEG_DONE
                elif failed:
                    f |= SEG_FAILED
                segs.append((f, vals, st[0] if st else 0, done[0] if f & SEG_DONE else 0))
        cols, comparable = _old_columns(self.kind, _old_status(source))
        return (flags | (0 if comparable else OBJ_OLD_OTHER), generation, observed, cols, segs)

    def arrays(self) -> dict:
        """The keyword arguments of runtime.sagg_args / Context.status_aggregate for the objects of ``device``."""
        self.device = [i for i in range(len(self.raw)) if i not in self.host]
        recs = [self.recs[i] for i in self.device]
        nv = 5 if self.kind == DEPLOYMENT else 3
        segs = [s for r in recs for s in r[4]]
        off = np.zeros(len(recs) + 1, np.int32)
        off[1:] = np.cumsum([len(r[4]) for r in recs])
        a = dict(kind=self.kind, obj_seg_off=off, obj_flags=np.array([r[0] for r in recs], np.uint8),
                 old_vals=np.array([r[3] for r in recs], np.int64).reshape(len(recs), 6 if self.kind == DEPLOYMENT else 5).T.copy(),
                 seg_vals=np.array([s[1] for s in segs], np.int32).reshape(len(segs), nv).T.copy(),
                 seg_flags=np.array([s[0] for s in segs], np.uint8))
        ca, cb = np.array([s[2] for s in segs], np.int64), np.array([s[3] for s in segs], np.int64)
        if self.kind == DEPLOYMENT:
            a.update(obj_generation=np.array([r[1] for r in recs], np.int64),
                     obj_observed=np.array([r[2] for r in recs], np.int64), seg_observed=ca, seg_synced=cb)
        else:
            a.update(seg_start=ca, seg_done=cb)
        return a

    def apply(self, r: Optional[dict], now: int = 0) -> List[Tuple[bool, Optional[StatusAggError]]]:
        """Write the results back into the source objects: ``status`` where it changed and, Deployment, the
        digests annotation; unchanged objects stay untouched. ``r``: kad_status_aggregate's outputs for
        ``device`` (None when it is empty). Returns per added object (needUpdate, error)."""
        out: List[Tuple[bool, Optional[StatusAggError]]] = [(False, None)] * len(self.raw)
        for i, e in self.errors.items():
            out[i] = (False, e)
        for i in self.host:
            if i not in self.errors:
                out[i] = self._host(i, now)
        for j, i in enumerate(self.device):
            if i in self.errors:
                continue
            source, _, cluster_objs = self.raw[i]
            changed = bool(r["changed"][j])
            sums = [int(v) for v in r["sums"][:, j]]
            if self.kind == DEPLOYMENT:
                if changed:
                    source["status"] = deployment_status(sums, int(r["observed"][j]))
                changed = _write_digests(source, cluster_objs) or changed
            else:
                cond, done = None, None
                if r["finished"][j]:
                    segs = self.recs[i][4]
                    names = list(cluster_objs)
                    cond = job_condition([n for n, s in zip(names, segs) if s[0] & SEG_DONE],
                                         [n for n, s in zip(names, segs) if s[0] & SEG_FAILED], now)
                    if r["n_failed"][j] == 0:
                        done = int(r["done_max"][j])
                old = self.raw[i][0].get("status")
                old_cond = old.get("conditions") if isinstance(old, dict) and "conditions" in old else None
                changed = changed or not deep_equal([cond] if cond else None, old_cond)
                if changed:
                    start = int(r["start_min"][j])
                    source["status"] = job_status(sums, None if start == NO_START else start, done, cond)
            out[i] = (changed, None)
        return out

    def _host(self, i: int, now: int) -> Tuple[bool, Optional[StatusAggError]]:
        source, fed, cluster_objs = self.raw[i]
        try:
            if self.kind == DEPLOYMENT:
                return aggregate_deployment(source, fed, cluster_objs, self.up_to_date[i]), None
            return aggregate_job(source, fed, cluster_objs, self.up_to_date[i], now), None
        except StatusAggError as e:
            return False, e


# ------------------------------------------------------------------ numpy restatement (cost comparison)
def sagg_numpy(kind: int, **a) -> dict:
    """kad_status_aggregate restated with numpy on one thread over the same arrays: what the cost script compares
    the device with. Inputs are assumed valid."""
    off = np.asarray(a["obj_seg_off"], np.int64)
    O, S = len(off) - 1, int(off[-1])
    nv = 5 if kind == DEPLOYMENT else 3
    of, sf = np.asarray(a["obj_flags"]), np.asarray(a["seg_flags"])
    n = np.diff(off)
    seg_obj = np.repeat(np.arange(O), n)
    err = (of & OBJ_ERROR) != 0
    live = ((sf & SEG_NIL) == 0) & ~err[seg_obj]
    vals = np.asarray(a["seg_vals"], np.int64).reshape(nv, S)
    old = np.asarray(a["old_vals"], np.int64).reshape(-1, O)
    sums = np.zeros((nv, O), np.int64)
    for v in range(nv):
        np.add.at(sums[v], seg_obj[live], vals[v][live])
    sums = sums.astype(np.uint64).astype(np.uint32).view(np.int32).reshape(nv, O)  # Go int32 wraps
    differ = ((of & OBJ_OLD_OTHER) != 0) | (sums.astype(np.int64) != old[:nv]).any(axis=0)
    out = {"sums": sums}
    if kind == DEPLOYMENT:
        stale = ((sf & SEG_NIL) != 0) | ((sf & SEG_SYNCED) == 0) | (np.asarray(a["seg_observed"]) != np.asarray(a["seg_synced"]))
        clear = np.zeros(O, bool)
        clear[seg_obj[stale]] = True
        keep = ((of & OBJ_UPTODATE) != 0) & ~clear
        obs = np.where(keep, a["obj_generation"], a["obj_observed"]).astype(np.int64)
        differ |= obs != old[5]
        out["observed"] = np.where(err, 0, obs)
    else:
        start, done = np.full(O, NO_START, np.int64), np.full(O, NO_DONE, np.int64)
        m = live & ((sf & SEG_START) != 0)
        np.minimum.at(start, seg_obj[m], np.asarray(a["seg_start"])[m])
        m = live & ((sf & SEG_DONE) != 0)
        np.maximum.at(done, seg_obj[m], np.asarray(a["seg_done"])[m])
        n_done = np.bincount(seg_obj[m], minlength=O).astype(np.int32)
        n_failed = np.bincount(seg_obj[live & ((sf & SEG_DONE) == 0) & ((sf & SEG_FAILED) != 0)], minlength=O).astype(np.int32)
        fin = n_done + n_failed
        finished = (fin > 0) & (fin == n)
        differ |= (start != old[3]) | (np.where(finished & (n_failed == 0), done, NO_DONE) != old[4])
        out.update(start_min=np.where(err, 0, start), done_max=np.where(err, 0, done), n_done=n_done, n_failed=n_failed,
                   finished=finished.astype(np.uint8))
    out["changed"] = (differ & ~err).astype(np.uint8)
    return out
