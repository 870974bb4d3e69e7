"""Rollout planning for a batch of federated Deployments: the host side of kad_rollout_plan.

While a Deployment rolls out across member clusters, the sync controller's managed dispatcher asks the rollout
planner, per member cluster, which replicas, maxSurge and maxUnavailable it may be given now, so that the federation
as a whole stays inside the template's own maxSurge / maxUnavailable (pkg/controllers/sync/dispatch/managed.go:
160-323, pkg/controllers/util/rolloutplan.go). This module restates everything around the numeric plan:

* ``get_value_from_int_or_percent`` / ``retrieve_fencepost`` — RetrieveFencepost, resolveFenceposts (:731-796);
* ``retrieve_new_replicaset_info`` (:798-829), ``target_info`` — unstructuredObjToTargetInfo (:364-447);
* ``new_planner`` — NewRolloutPlanner (:459-487); ``replicas_override_for_cluster`` / ``total_replicas``
  (pkg/controllers/sync/resource.go:392-427);
* ``RolloutBatch`` — the driver (managed.go:163-213, 296-320) packing objects into kad_rollout_plan's columns and
  turning its outputs back into plans, overrides (RolloutPlan.toOverrides, :79-91) and actions;
* ``plan_numpy`` — Plan() (:569-695) itself in the prefix-sum form the device uses, over the same columns, for the
  objects where nothing can wrap (``nowrap``).
"""

from __future__ import annotations

import math
from typing import Dict, List, Optional, Sequence

import numpy as np

REPLICA_PATH = "/spec/replicas"
MAX_SURGE_PATH = "/spec/strategy/rollingUpdate/maxSurge"
MAX_UNAVAILABLE_PATH = "/spec/strategy/rollingUpdate/maxUnavailable"
MAX_SURGE_FIELDS = ("spec", "strategy", "rollingUpdate", "maxSurge")
MAX_UNAVAILABLE_FIELDS = ("spec", "strategy", "rollingUpdate", "maxUnavailable")
TEMPLATE_PREFIX = ("spec", "template")
PREFIX = "kubeadmiral.io/"
CURRENT_REVISION_ANNOTATION = PREFIX + "current-revision"
LAST_REPLICASET_NAME = PREFIX + "last-replicaset-name"
LATEST_RS_NAME = "latestreplicaset.kubeadmiral.io/name"
LATEST_RS_REPLICAS = "latestreplicaset.kubeadmiral.io/replicas"
LATEST_RS_AVAILABLE = "latestreplicaset.kubeadmiral.io/available-replicas"

# kad_rollout_plan's constants (include/kad_sched.h)
FIELDS = ("replicas", "actual", "available", "updated_replicas", "updated_available", "current_new",
          "current_new_available", "max_surge", "max_unavailable", "desired")  # the rows of tgt_vals
NV = len(FIELDS)
OBJ_ERROR = 1
TGT_UPDATED, TGT_EXISTS, TGT_TO_DELETE = 1, 2, 4
PLANNED, HAS_REPLICAS, HAS_SURGE, HAS_UNAVAILABLE, ONLY_PATCH_REPLICAS = 1, 2, 4, 8, 16
ACT_KEEP_TEMPLATE_PATCH, ACT_NONE, ACT_DELETE, ACT_CREATE, ACT_PATCH_REPLICAS, ACT_UPDATE = range(6)
ACTION_NAMES = ("keep-template-patch", "none", "delete", "create", "patch-replicas", "update")
ST_OK, ST_SCALE, ST_INVALID, ST_ERROR = range(4)
NOWRAP_BELOW = 1 << 29  # csrc/kad_rollout.h RO_NOWRAP_BELOW


class RolloutError(Exception):
    """An error the reference returns from planRolloutProcess (recorded as PlanRolloutFailed)."""


def _i32(v: int) -> int:
    return (int(v) + 2 ** 31) % 2 ** 32 - 2 ** 31


# ------------------------------------------------------------------ unstructured access
def _nested(obj: dict, fields: Sequence[str]):
    """unstructured.NestedFieldNoCopy → (value, found); a non-map on the way is an error."""
    cur = obj
    for k, f in enumerate(fields):
        if not isinstance(cur, dict):
            raise RolloutError(f"{'.'.join(fields[:k])} accessor error: {cur!r} is not a map")
        if f not in cur:
            return None, False
        cur = cur[f]
    return cur, True


def _is_int(v) -> bool:
    return isinstance(v, int) and not isinstance(v, bool)


def nested_int64(obj: dict, fields: Sequence[str]) -> Optional[int]:
    """unstructured.NestedInt64 as GetInt64FromPath uses it: None when absent, an error for another type (a JSON
    number with a fraction or an exponent decodes to float64 in Go and is one)."""
    v, found = _nested(obj, fields)
    if not found:
        return None
    if not _is_int(v):
        raise RolloutError(f"{'.'.join(fields)} accessor error: {v!r} is not an int64")
    return v


def split_dot_path(path: str, prefix: Sequence[str] = ()) -> List[str]:
    return list(prefix) + [p for p in path.split(".") if p]


def _annotations(obj: dict) -> dict:
    a = (obj.get("metadata") or {}).get("annotations")
    return a if isinstance(a, dict) else {}


# ------------------------------------------------------------------ fenceposts
def get_value_from_int_or_percent(value, total: int, round_up: bool) -> int:
    """intstr.GetValueFromIntOrPercent, restated without its source at hand (DESIGN §4 lists it as unpinned
    third-party semantics): an int is itself; a string must end in ``%`` with an Atoi-parseable rest, and is
    ceil / floor of float64(v) * float64(total) / 100."""
    if _is_int(value):
        return value
    s = str(value)
    if not s.endswith("%"):
        raise RolloutError(f"invalid value for IntOrString: invalid type: string is not a percentage: {s!r}")
    body = s[:-1]
    digits = body[1:] if body[:1] in "+-" else body
    if not digits or not digits.isascii() or not digits.isdigit():
        raise RolloutError(f"invalid value for IntOrString: invalid value {s!r}")
    x = float(int(body)) * float(total) / 100
    return int(math.ceil(x) if round_up else math.floor(x))


def _int_or_string(obj: dict, fields: Sequence[str]):
    """The string value first, then the int64 one (:764-783); neither: the default 0."""
    try:
        v, found = _nested(obj, fields)
    except RolloutError:
        return 0
    if found and isinstance(v, str):
        return v
    if found and _is_int(v):
        return _i32(v)
    return 0


def retrieve_fencepost(obj: dict, surge_fields: Sequence[str], unavailable_fields: Sequence[str], replicas: int):
    """RetrieveFencepost (:760-796) → (maxSurge, maxUnavailable): surge rounds up, unavailable down, both zero
    makes unavailable 1, negatives clamp to 0."""
    surge = get_value_from_int_or_percent(_int_or_string(obj, surge_fields), replicas, True)
    unavailable = get_value_from_int_or_percent(_int_or_string(obj, unavailable_fields), replicas, False)
    if surge == 0 and unavailable == 0:
        unavailable = 1
    return max(_i32(surge), 0), max(_i32(unavailable), 0)


def _parse_int32(s: str) -> int:
    """strconv.ParseInt(s, 10, 32)."""
    body = s[1:] if s[:1] in "+-" else s
    if not body or not body.isascii() or not body.isdigit():
        raise RolloutError(f'strconv.ParseInt: parsing "{s}": invalid syntax')
    v = int(s)
    if not -2 ** 31 <= v < 2 ** 31:
        raise RolloutError(f'strconv.ParseInt: parsing "{s}": value out of range')
    return v


def retrieve_new_replicaset_info(obj: dict):
    """retrieveNewReplicaSetInfo (:798-829) → (replicas, availableReplicas) of the latest replica set, both 0 when
    its name is the last-replicaset-name annotation's (the annotations lag behind the template)."""
    ann = _annotations(obj)
    for key in (LATEST_RS_REPLICAS, LATEST_RS_AVAILABLE):
        if not ann.get(key):
            raise RolloutError(f"missing annotation {key}")
        if key == LATEST_RS_REPLICAS:
            replicas = _parse_int32(ann[key])
        else:
            available = _parse_int32(ann[key])
    if LATEST_RS_NAME not in ann:
        raise RolloutError(f"missing annotation {LATEST_RS_NAME}")
    if LAST_REPLICASET_NAME in ann and ann[LAST_REPLICASET_NAME] == ann[LATEST_RS_NAME]:
        return 0, 0
    return replicas, available


def target_info(cluster: str, obj: Optional[dict], desired: int, desired_revision: str, ftc) -> dict:
    """unstructuredObjToTargetInfo (:364-447) → the target as a dict of FIELDS, ``name``, ``updated``, ``exists``.
    ActualReplicas is read from the ReplicasSpec path a second time, as the reference does (:404-415): it is the
    spec's replicas, not status.replicas."""
    t = {f: 0 for f in FIELDS}
    t.update(name=cluster, updated=False, exists=obj is not None, desired=_i32(desired))
    if obj is None:
        return t
    try:
        replicas = nested_int64(obj, split_dot_path(ftc.replicas_spec))
    except RolloutError as e:
        raise RolloutError(f"failed to retrieve replicas, err: {e}") from None
    if replicas is None:
        raise RolloutError("failed to retrieve replicas, err: <nil>")
    try:
        ms, mu = retrieve_fencepost(obj, MAX_SURGE_FIELDS, MAX_UNAVAILABLE_FIELDS, _i32(replicas))
    except RolloutError as e:
        raise RolloutError(f"failed to retrieve fencepost: {e}") from None
    ann = _annotations(obj)
    if CURRENT_REVISION_ANNOTATION not in ann:
        raise RolloutError(f"failed to retrieve annotation {CURRENT_REVISION_ANNOTATION}")
    updated = ann[CURRENT_REVISION_ANNOTATION] == desired_revision
    try:
        cur_new, cur_new_avail = retrieve_new_replicaset_info(obj)
    except RolloutError as e:
        raise RolloutError(f"failed to retrieve new replicaSet info: {e}") from None
    try:
        actual = nested_int64(obj, split_dot_path(ftc.replicas_spec))
    except RolloutError as e:
        raise RolloutError(f"failed to retrieve actual replicas: {e}") from None
    try:
        available = nested_int64(obj, split_dot_path(ftc.available_replicas_status))
    except RolloutError as e:
        raise RolloutError(f"failed to retrieve actual available replicas: {e}") from None
    t.update(replicas=_i32(replicas), actual=_i32(actual or 0), available=_i32(available or 0),
             updated_replicas=cur_new if updated else 0, updated_available=cur_new_avail if updated else 0,
             current_new=cur_new, current_new_available=cur_new_avail, updated=updated, max_surge=ms, max_unavailable=mu)
    return t


def new_planner(fed: dict, replicas: int):
    """NewRolloutPlanner (:459-487) → (maxSurge, maxUnavailable, desired revision) of the federated object."""
    try:
        ms, mu = retrieve_fencepost(fed, TEMPLATE_PREFIX + MAX_SURGE_FIELDS, TEMPLATE_PREFIX + MAX_UNAVAILABLE_FIELDS, replicas)
    except RolloutError as e:
        raise RolloutError(f"failed to retrieve maxSurge or maxUnavailable from federated resource: {e}") from None
    ann = _annotations(fed)
    if CURRENT_REVISION_ANNOTATION not in ann:
        raise RolloutError(f"failed to retrieve annotation {CURRENT_REVISION_ANNOTATION} from federated resource")
    return ms, mu, ann[CURRENT_REVISION_ANNOTATION]


# ------------------------------------------------------------------ the federated object's replicas
def overrides_map(fed: dict, controller_order: Sequence[str] = ()) -> Dict[str, list]:
    """overridesForCluster (sync/resource.go:341-388): every controller's patches per cluster, the controllers the
    type config lists first and in its order (a stable sort), the others after them as they stand."""
    overrides = (fed.get("spec") or {}).get("overrides") or []
    rank = {c: i for i, c in enumerate(controller_order)}
    ordered = sorted(overrides, key=lambda o: rank.get(o.get("controller"), len(rank)))
    out: Dict[str, list] = {}
    for o in ordered:
        for c in o.get("clusters") or []:
            out.setdefault(c.get("clusterName"), []).extend(c.get("patches") or [])
    return out


def replicas_override_for_cluster(fed: dict, ftc, cluster: str, omap: Optional[Dict[str, list]] = None) -> int:
    """ReplicasOverrideForCluster (sync/resource.go:392-415): the first /spec/replicas patch with a value, which must
    be a JSON number (float64, truncated to int32), else the template's replicas."""
    omap = overrides_map(fed) if omap is None else omap
    for p in omap.get(cluster, []):
        if p.get("path") == REPLICA_PATH and p.get("value") is not None:
            v = p["value"]
            if isinstance(v, bool) or not isinstance(v, (int, float)):
                raise RolloutError(f"failed to retrieve replicas override for {cluster}")
            return _i32(int(v))
    default = nested_int64(fed, split_dot_path(ftc.replicas_spec, TEMPLATE_PREFIX))
    if default is None:
        raise RolloutError(f"failed to retrieve replicas override for {cluster}")
    return _i32(default)


def total_replicas(fed: dict, ftc, clusters, omap: Optional[Dict[str, list]] = None) -> int:
    """TotalReplicas (sync/resource.go:417-427), a wrapping int32 sum."""
    omap = overrides_map(fed) if omap is None else omap
    total = 0
    for c in clusters:
        total = _i32(total + replicas_override_for_cluster(fed, ftc, c, omap))
    return total


def check_retain_replicas(fed: dict) -> bool:
    """checkRetainReplicas (dispatch/retain.go:527-533)."""
    v, found = _nested(fed, ("spec", "retainReplicas"))
    if found and not isinstance(v, bool):
        raise RolloutError(f"spec.retainReplicas accessor error: {v!r} is not a bool")
    return bool(found and v)


def to_overrides(plan: Optional[dict]) -> list:
    """RolloutPlan.toOverrides (:79-91); no plan: no patches (GetRolloutOverrides, :124-130)."""
    out = []
    if plan is None:
        return out
    for key, path in (("replicas", REPLICA_PATH), ("max_surge", MAX_SURGE_PATH), ("max_unavailable", MAX_UNAVAILABLE_PATH)):
        if plan[key] is not None:
            out.append({"path": path, "value": plan[key]})
    return out


# ------------------------------------------------------------------ Plan() over the columns
def nowrap(obj_tgt_off, obj_max_surge, obj_max_unavailable, obj_replicas, tgt_vals, **_) -> np.ndarray:
    """bool[O]: the absolute values of the object's inputs sum to less than 2^29, so nothing in Plan() wraps int32
    (a budget is bounded by twice that sum, a budget plus a least surge by three times, a budget less every offer
    by four times) and the prefix-sum form is exact."""
    off = np.asarray(obj_tgt_off, np.int64)
    O = len(off) - 1
    total = sum(np.abs(np.asarray(a, np.int64)) for a in (obj_max_surge, obj_max_unavailable, obj_replicas))
    total = np.asarray(total, np.int64).reshape(O)
    T = int(off[-1]) if O >= 0 and len(off) else 0
    if T:
        per = np.abs(np.asarray(tgt_vals, np.int64).reshape(NV, T)).sum(axis=0)
        csum = np.concatenate(([0], np.cumsum(per)))
        total = total + (csum[off[1:]] - csum[off[:-1]])
    return total < NOWRAP_BELOW


def plan_numpy(obj_tgt_off, obj_max_surge, obj_max_unavailable, obj_replicas, obj_flags, tgt_vals, tgt_flags) -> dict:
    """kad_rollout_plan's outputs in the prefix-sum form: in every pass a target takes min(budget, its offer) from a
    positive budget and nothing otherwise, so the budget it sees is m0 if m0 <= 0 and max(m0 - the offers before
    it, 0) otherwise. Exact only where nothing wraps: raises ValueError for a live object that ``nowrap`` rejects."""
    off = np.asarray(obj_tgt_off, np.int64)
    O, T = len(off) - 1, len(np.asarray(tgt_flags))
    of = np.asarray(obj_flags, np.uint8).reshape(O)
    tf = np.asarray(tgt_flags, np.uint8).reshape(T)
    v = np.asarray(tgt_vals, np.int64).reshape(NV, T) if T else np.zeros((NV, 0), np.int64)
    live = (of & OBJ_ERROR) == 0
    ok = nowrap(off, obj_max_surge, obj_max_unavailable, obj_replicas, v)
    if (live & ~ok).any():
        raise ValueError("plan_numpy: an object's inputs may wrap int32; only the serial walk plans it")
    obj = np.repeat(np.arange(O), np.diff(off))
    p_ms, p_mu, p_rep = (np.asarray(a, np.int64).reshape(O) for a in (obj_max_surge, obj_max_unavailable, obj_replicas))
    r, act, av, ur, uar, cn, cna, ms, mu, d = v
    upd = (tf & TGT_UPDATED) != 0
    pos = lambda x: np.maximum(x, 0)  # noqa: E731
    rtu, rtua = pos(r - ur), pos(r - uar)
    during = (cn < r) | (upd & (rtu > 0))
    ls, lu = pos(act - r), pos(r - av)
    ls = np.where(during, np.maximum(ls, np.minimum(ms, ls + pos(r - cn))), ls)
    lu = np.where(during, np.maximum(lu, np.minimum(mu, pos(r - cna))), lu)
    c_out, c_in, c_upd = d > r, d < r, d == r
    p_surge = (p_ms != 0) & (p_mu == 0)
    is_surge = (ms != 0) & (mu == 0)
    completed = rtu == 0
    flip = is_surge & ~p_surge[obj] & (rtua > 0)

    def osum(x):  # per object; every sum stays below 2^31 here, exact in float64
        return np.bincount(obj, weights=x, minlength=O).astype(np.int64)

    def before(a):  # the offers of the object's earlier targets, and the object's total
        c = np.cumsum(a) - a
        start = np.concatenate(([0], np.cumsum(a)))[off[:-1]]
        return c - start[obj], osum(a)

    def budget(m0, used):
        return np.where(m0 <= 0, m0, np.maximum(m0 - used, 0))

    def fence(m, least, to, cur):
        res = pos(np.minimum(m + least, to))
        return np.where((m < 0) & (least > cur) & (res > cur), cur, res)

    scaling = ((osum(c_out.astype(np.int64)) != 0) != (osum(c_in.astype(np.int64)) != 0)) & \
        (osum((~(completed & ~flip)).astype(np.int64)) == 0)
    cur = osum(r)
    S0 = (p_ms - (cur - p_rep) - osum(ls))[obj]
    U0 = (p_mu - (p_rep - cur) - osum(lu))[obj]
    ls_idle, lu_idle = np.where(during, 0, ls), np.where(during, 0, lu)
    x1s, T1s = before(np.where(c_out, pos(rtu - ls), 0))
    x1u, T1u = before(np.where(c_out, pos(rtua - lu), 0))
    x2u, T2u = before(np.where(c_in, pos(np.minimum(r - d, r) - lu_idle), 0))
    x3s, T3s = before(np.where(c_upd, pos(rtu - ls), 0))
    x3u, T3u = before(np.where(c_upd, pos(rtua - lu), 0))
    may_out = c_out & (upd | (r == 0))
    x4s, T4s = before(np.where(may_out, pos(d - r - ls_idle), 0))
    # passes 1 and 3: the fenceposts of the targets to scale out / to update
    S13 = budget(S0, np.where(c_out, x1s, T1s[obj] + x3s))
    U13 = budget(U0, np.where(c_out, x1u, (T1u + T2u)[obj] + x3u))
    skip13 = (S13 <= 0) & (U13 <= 0) & ~upd & ~during & (ls <= 0) & (lu <= 0)
    # pass 2
    U2 = budget(U0, T1u[obj] + x2u)
    in2 = c_in & ~((U2 <= 0) & (lu <= 0))
    res2 = pos(np.minimum(np.minimum(U2 + lu_idle, r - d), r))
    # pass 4
    S4 = budget(S0, (T1s + T3s)[obj] + x4s)
    out4 = may_out & ~((S4 <= 0) & (ls <= 0))
    res4 = pos(np.minimum(S4 + ls_idle, d - r))
    # pass 5
    r5 = np.where(in2, r - res2, r)
    lu5 = np.where(during, lu, pos(lu - (r - r5)))
    x5s, _ = before(np.where(c_in, pos(rtu - ls), 0))
    x5u, _ = before(np.where(c_in, pos(rtua - lu5), 0))
    S5 = budget(S0, (T1s + T3s + T4s)[obj] + x5s)
    U5 = budget(U0, (T1u + T2u + T3u)[obj] + x5u)
    skip5 = (S5 <= 0) & (U5 <= 0) & ~upd & ~during & ~(lu5 > 0)  # (its least surge is 0: desired < replicas)
    fenced = np.where(c_in, ~skip5, ~skip13)
    S = np.where(c_in, S5, S13)
    U = np.where(c_in, U5, U13)
    s = fence(S, ls, rtu, ms)
    u = fence(U, np.where(c_in, lu5, lu), rtua, mu)
    final = completed & ~flip  # correctFencepost
    both0 = (s == 0) & (u == 0) & ~final
    s = np.where(both0 & is_surge, 1, s)
    u = np.where(both0 & ~is_surge, 1, u)
    has_su = fenced & ~final
    planned = fenced | in2 | out4
    has_r = (c_out & (fenced | out4)) | (c_in & (fenced | in2))
    rep = np.where(c_out, np.where(out4, r + res4, r), r5)
    only = c_in & in2 & ~fenced
    # validatePlans
    counted = np.where(planned, np.where(has_r, rep, d), r)
    n_planned, desired = osum(counted), osum(d)
    lo, hi = np.minimum(desired, cur), np.maximum(desired, cur)
    invalid = ~scaling & ((p_rep - desired > p_mu) | (lo - n_planned > p_mu) | (n_planned - hi > p_ms))
    dead = (~live | invalid)[obj]
    sc = scaling[obj] & ~dead
    planned = np.where(sc, True, planned & ~dead)
    has_r, has_su, only = (x & ~dead & ~sc for x in (has_r, has_su, only))
    flags = (planned * PLANNED + has_r * HAS_REPLICAS + has_su * (HAS_SURGE | HAS_UNAVAILABLE) + only * ONLY_PATCH_REPLICAS)
    rep = np.where(has_r, rep, 0)
    exists, to_del = (tf & TGT_EXISTS) != 0, (tf & TGT_TO_DELETE) != 0
    action = np.where(~planned, np.where(exists, ACT_KEEP_TEMPLATE_PATCH, ACT_NONE),
                      np.where(to_del & (~has_r | (rep == 0)), ACT_DELETE,
                               np.where(~exists, ACT_CREATE, np.where(only & has_r, ACT_PATCH_REPLICAS, ACT_UPDATE))))
    status = np.where(~live, ST_ERROR, np.where(scaling, ST_SCALE, np.where(invalid, ST_INVALID, ST_OK)))
    return {"replicas": rep.astype(np.int32), "max_surge": np.where(has_su, s, 0).astype(np.int32),
            "max_unavailable": np.where(has_su, u, 0).astype(np.int32), "plan_flags": flags.astype(np.uint8),
            "action": action.astype(np.uint8), "status": status.astype(np.uint8)}


def plans_of(result: dict, lo: int, hi: int, names: Sequence[str]) -> Dict[str, dict]:
    """The reference's RolloutPlans of one object from kad_rollout_plan's outputs for its targets [lo, hi)."""
    out = {}
    for i, name in zip(range(lo, hi), names):
        f = int(result["plan_flags"][i])
        if f & PLANNED:
            out[name] = {"replicas": int(result["replicas"][i]) if f & HAS_REPLICAS else None,
                         "max_surge": int(result["max_surge"][i]) if f & HAS_SURGE else None,
                         "max_unavailable": int(result["max_unavailable"][i]) if f & HAS_UNAVAILABLE else None,
                         "only_patch_replicas": bool(f & ONLY_PATCH_REPLICAS)}
    return out


# ------------------------------------------------------------------ the batch
class RolloutOutcome:
    """One object's answer: ``status`` (ST_*), ``plans`` (cluster → plan dict, the reference's RolloutPlans),
    ``overrides`` (cluster → patches, GetRolloutOverrides), ``actions`` (cluster → ACT_*), ``error``."""

    __slots__ = ("status", "plans", "overrides", "actions", "error")

    def __init__(self, status, plans, overrides, actions, error=None):
        self.status, self.plans, self.overrides, self.actions, self.error = status, plans, overrides, actions, error


class RolloutBatch:
    """Objects packed into kad_rollout_plan's columns. ``add`` runs the driver's host half for one federated object
    (managed.go:163-213, 296-320); a host error makes it an ERROR object, which the device passes through: the
    member objects that exist are patched with their template kept (:229-235)."""

    def __init__(self, ftc, controller_order: Sequence[str] = ()):
        self.ftc, self.controller_order = ftc, tuple(controller_order)
        self.off = [0]
        self.obj = []      # (max_surge, max_unavailable, replicas, flags)
        self.targets = []  # dicts of target_info, in each object's sorted order
        self.errors: List[Optional[str]] = []

    def __len__(self):
        return len(self.obj)

    def add(self, fed: dict, member_objs: Dict[str, Optional[dict]], selected) -> None:
        """``member_objs``: the object's copy (or None) in every ready cluster it could be fetched from;
        ``selected``: the names of the clusters placement selects."""
        selected = set(selected)
        cluster_objs, to_delete = {}, set()
        for name, obj in member_objs.items():
            if name not in selected:
                if obj is None or (obj.get("metadata") or {}).get("deletionTimestamp") is not None:
                    continue
                to_delete.add(name)
            cluster_objs[name] = obj
        names = sorted(cluster_objs, key=lambda s: s.encode())  # sortTargets (:699)
        err, ms, mu, replicas, ts = None, 0, 0, 0, None
        try:
            if (self.ftc.group, self.ftc.version, self.ftc.kind) != ("apps", "v1", "Deployment"):
                raise RolloutError(f"Unsupported target type for rollout plan: {self.ftc.group}/{self.ftc.version}, "
                                   f"Kind={self.ftc.kind}")
            omap = overrides_map(fed, self.controller_order)
            replicas = total_replicas(fed, self.ftc, selected, omap)
            ms, mu, revision = new_planner(fed, replicas)
            ts = []
            for name in names:
                desired = 0 if name in to_delete else replicas_override_for_cluster(fed, self.ftc, name, omap)
                try:
                    ts.append(target_info(name, cluster_objs[name], desired, revision, self.ftc))
                except RolloutError as e:
                    raise RolloutError(f"Failed to register target in {name}: {e}") from None
        except RolloutError as e:
            err = str(e)
        if err is not None:  # the device reads none of it, but the actions need EXISTS
            ts = [dict({f: 0 for f in FIELDS}, name=n, updated=False, exists=cluster_objs[n] is not None) for n in names]
            ms = mu = replicas = 0
        for t in ts:
            t["to_delete"] = t["name"] in to_delete and err is None
        self.targets += ts
        self.off.append(len(self.targets))
        self.obj.append((ms, mu, replicas, OBJ_ERROR if err is not None else 0))
        self.errors.append(err)

    def arrays(self) -> dict:
        O, T = len(self.obj), len(self.targets)
        o = np.array(self.obj, np.int64).reshape(O, 4)
        vals = np.zeros((NV, T), np.int32)
        flags = np.zeros(T, np.uint8)
        for i, t in enumerate(self.targets):
            vals[:, i] = [t[f] for f in FIELDS]
            flags[i] = (TGT_UPDATED if t["updated"] else 0) | (TGT_EXISTS if t["exists"] else 0) | \
                (TGT_TO_DELETE if t["to_delete"] else 0)
        return {"obj_tgt_off": np.array(self.off, np.int32), "obj_max_surge": o[:, 0].astype(np.int32),
                "obj_max_unavailable": o[:, 1].astype(np.int32), "obj_replicas": o[:, 2].astype(np.int32),
                "obj_flags": o[:, 3].astype(np.uint8), "tgt_vals": vals, "tgt_flags": flags}

    def apply(self, result: dict) -> List[RolloutOutcome]:
        out = []
        for k in range(len(self.obj)):
            lo, hi = self.off[k], self.off[k + 1]
            names = [t["name"] for t in self.targets[lo:hi]]
            plans = plans_of(result, lo, hi, names)
            out.append(RolloutOutcome(int(result["status"][k]), plans, {n: to_overrides(plans.get(n)) for n in names},
                                      {n: int(result["action"][i]) for i, n in zip(range(lo, hi), names)}, self.errors[k]))
        return out
