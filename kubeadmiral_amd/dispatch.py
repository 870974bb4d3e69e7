"""Sync dispatch planning for a batch of federated objects: the host side of kad_dispatch_plan.

Every reconcile of a federated object ends in the sync controller's ``syncToClusters``
(pkg/controllers/sync/controller.go:425-544): the placement is computed (sync/placement.go:45-116,
resource.go:170-175) and, for every joined cluster, the loop decides whether the member object is created, updated,
deleted, orphaned or left alone and which propagation status the cluster gets before anything is dispatched. This
module restates everything around that loop:

* ``cluster_flags_of`` — IsClusterReady (util/federatedinformer.go:292-301), the deletion timestamp,
  IsCascadingDeleteEnabled (util/cascadingdeleteannotation.go:29-40) and the cascading-delete finalizer
  (``cascading_delete_finalizer``, controller.go:203-216) of a FederatedCluster given as a dict;
* ``orphaning_behavior`` — GetOrphaningBehavior (util/orphaningannotation.go:48-62);
* ``DispatchBatch`` — objects, federated namespaces and the informers' member objects packed into
  kad_dispatch_plan's arrays, and its outputs turned back into names (``apply``);
* ``plan_numpy`` — the loop itself, vectorised over sorted (object, cluster) keys, over the same arrays.

ObjectNeedsUpdate, Wait()'s status transitions, the propagated versions and SetFederatedStatus are syncfin.py's
(kad_sync_needs_update, kad_sync_finish). Deleting objects (ensureDeletion) and the operations themselves are the
caller's.
"""

from __future__ import annotations

from typing import Dict, List, Optional, Sequence, Set

import numpy as np

from . import objects as O

PREFIX = "kubeadmiral.io/"
INTERNAL_PREFIX = "internal." + PREFIX
CASCADING_DELETE_ANNOTATION = PREFIX + "cascading-delete"
FINALIZER_CASCADING_DELETE_PREFIX = PREFIX + "cascading-delete"
ORPHAN_ANNOTATION = PREFIX + "orphan"
ORPHAN_INTERNAL_ANNOTATION = INTERNAL_PREFIX + "orphan"
ADOPTED_ANNOTATION = PREFIX + "adopted"
ORPHAN_ALL, ORPHAN_ADOPTED, ORPHAN_NONE = "all", "adopted", ""

# kad_dispatch_plan's constants (include/kad_sched.h)
MAX_CLUSTERS = 16384
CL_READY, CL_TERMINATING, CL_CASCADING, CL_FINALIZER = 1, 2, 4, 8
OBJ_ERROR, OBJ_ORPHAN_ALL, OBJ_ORPHAN_ADOPTED = 1, 2, 4
OB_EXISTS, OB_DELETING, OB_ADOPTED, OB_RETRIEVAL_FAILED = 1, 2, 4, 8
NS_NONE, NS_UNFEDERATED = -1, -2
OP_NONE, OP_CREATE, OP_UPDATE, OP_DELETE, OP_REMOVE_LABEL = range(5)
OP_NAMES = ("none", "create", "update", "delete", "remove-label")
(ST_NONE, ST_CLUSTER_NOT_READY, ST_CACHED_RETRIEVAL_FAILED, ST_WAITING_FOR_REMOVAL, ST_LABEL_REMOVAL_TIMED_OUT,
 ST_DELETION_TIMED_OUT, ST_CLUSTER_TERMINATING, ST_FINALIZER_CHECK_FAILED, ST_CREATION_TIMED_OUT,
 ST_UPDATE_TIMED_OUT) = range(10)
STATUS_NAMES = ("", "ClusterNotReady", "CachedRetrievalFailed", "WaitingForRemoval", "LabelRemovalTimedOut",
                "DeletionTimedOut", "ClusterTerminating", "FinalizerCheckFailed", "CreationTimedOut", "UpdateTimedOut")
RES_RECHECK, RES_PLACEMENT_FAILED = 1, 2
COMPUTE_PLACEMENT_FAILED = "ComputePlacementFailed"


def _fnv32(data: bytes) -> int:
    """hash/fnv New32 (FNV-1)."""
    h = 2166136261
    for b in data:
        h = (h * 16777619) & 0xFFFFFFFF
        h ^= b
    return h


def cascading_delete_finalizer(ftc_name: str) -> str:
    """The sync controller's per-type finalizer on a FederatedCluster (controller.go:203-216)."""
    raw = ftc_name.encode()
    return f"{FINALIZER_CASCADING_DELETE_PREFIX}-{raw[:20].decode(errors='ignore')}-{_fnv32(raw)}"


def _meta(obj: Optional[dict]) -> dict:
    m = obj.get("metadata") if isinstance(obj, dict) else None
    return m if isinstance(m, dict) else {}


def _annotations(obj: Optional[dict]) -> dict:
    a = _meta(obj).get("annotations")
    return a if isinstance(a, dict) else {}


def cluster_flags_of(cluster: dict, finalizer: str) -> int:
    """The four facts syncToClusters reads from a FederatedCluster (a dict: types.FederatedCluster has none of
    them): a Ready condition with status True, a deletion timestamp, the cascading-delete annotation, the sync
    controller's finalizer."""
    f = 0
    status = cluster.get("status") if isinstance(cluster.get("status"), dict) else {}
    for cond in status.get("conditions") or []:
        if isinstance(cond, dict) and cond.get("type") == "Ready" and cond.get("status") == "True":
            f |= CL_READY
            break
    if _meta(cluster).get("deletionTimestamp") is not None:
        f |= CL_TERMINATING
    if CASCADING_DELETE_ANNOTATION in _annotations(cluster):
        f |= CL_CASCADING
    if finalizer in (_meta(cluster).get("finalizers") or []):
        f |= CL_FINALIZER
    return f


def orphaning_behavior(obj: dict) -> str:
    """GetOrphaningBehavior: the internal annotation wins where it exists, whatever it says."""
    ann = _annotations(obj)
    value = ann[ORPHAN_INTERNAL_ANNOTATION] if ORPHAN_INTERNAL_ANNOTATION in ann else ann.get(ORPHAN_ANNOTATION, "")
    return value if value in (ORPHAN_ALL, ORPHAN_ADOPTED) else ORPHAN_NONE


def observation_flags(member) -> int:
    """One informer lookup (util.GetClusterObject): the member object, None, or the error it failed with."""
    if member is None:
        return 0
    if isinstance(member, BaseException):
        return OB_RETRIEVAL_FAILED
    f = OB_EXISTS
    if _meta(member).get("deletionTimestamp") is not None:
        f |= OB_DELETING
    if _annotations(member).get(ADOPTED_ANNOTATION) == "true":
        f |= OB_ADOPTED
    return f


def placement_names(obj: dict) -> List[str]:
    """selectedClusterNames (placement.go:90-108) before the set is formed: every controller's cluster names in the
    object's own order. Raises objects.ObjectError where UnmarshalGenericPlacements fails."""
    return [c.name for p in (O._unmarshal_placements(obj).spec.placements or []) for c in (p.placement.clusters or [])]


class DispatchOutcome:
    """One object's answer: ``selected`` (the computed placement, names), ``ops`` (cluster → OP_*, the operations
    started), ``status`` (cluster → propagation status string), ``to_delete`` (the clusters whose member object is
    deleted or orphaned), ``recheck`` (shouldRecheckAfterDispatch), ``reason`` (ComputePlacementFailed or None) and
    ``rollout_members`` (cluster → member object or None over the ready clusters whose lookup did not fail and that
    are selected or hold the object: with ``selected``, what reconcile_rollout accepts)."""

    __slots__ = ("selected", "ops", "status", "to_delete", "recheck", "reason", "rollout_members")

    def __init__(self, selected, ops, status, to_delete, recheck, reason, rollout_members):
        self.selected, self.ops, self.status, self.to_delete = selected, ops, status, to_delete
        self.recheck, self.reason, self.rollout_members = recheck, reason, rollout_members


class DispatchBatch:
    """Objects packed into kad_dispatch_plan's arrays. ``clusters``: the joined FederatedCluster objects as dicts, in
    the order that gives the cluster ids; ``finalizer``: the sync controller's cascading-delete finalizer
    (:func:`cascading_delete_finalizer`); ``fed_namespaces``: federated namespace objects by namespace name (a row
    of the namespace table each, built on first use); ``limited_scope``: KubeFed targets a single namespace."""

    def __init__(self, type_config, clusters: Sequence[dict], finalizer: str,
                 fed_namespaces: Optional[Dict[str, dict]] = None, limited_scope: bool = False):
        self.ftc, self.limited_scope = type_config, limited_scope
        self.names = [_meta(c).get("name", "") for c in clusters]
        if len(self.names) > MAX_CLUSTERS:
            raise ValueError(f"kad_dispatch_plan covers at most {MAX_CLUSTERS} joined clusters")
        self.ids = {n: i for i, n in enumerate(self.names)}
        self.cluster_flags = np.array([cluster_flags_of(c, finalizer) for c in clusters], np.uint8)
        self.fed_namespaces = fed_namespaces or {}
        self.ns_row: Dict[str, int] = {}     # namespace name → row, -1 for one whose placement does not unmarshal
        self.ns_off, self.ns_cluster = [0], []
        self.obj_flags, self.obj_ns = [], []
        self.pl_off, self.pl_cluster = [0], []
        self.ob_off, self.ob_cluster, self.ob_flags = [0], [], []
        self.members: List[Dict[str, object]] = []
        self.errors: List[Optional[str]] = []

    def __len__(self):
        return len(self.obj_flags)

    def _ids_of(self, names: Sequence[str]) -> List[int]:
        return [self.ids.get(n, -1) for n in names]  # -1: not a joined cluster (computePlacement's intersection)

    def _namespace_row(self, ns_name: str) -> int:
        if ns_name not in self.ns_row:
            try:
                ids = self._ids_of(placement_names(self.fed_namespaces[ns_name]))
            except O.ObjectError:
                self.ns_row[ns_name] = -1
            else:
                self.ns_row[ns_name] = len(self.ns_off) - 1
                self.ns_cluster += ids
                self.ns_off.append(len(self.ns_cluster))
        return self.ns_row[ns_name]

    def add(self, fed: dict, member_objs: Dict[str, object]) -> None:
        """``member_objs``: per joined cluster name the informer's member object, None (or no key) where it holds
        none, or the exception the lookup failed with."""
        flags, ns, ids, err = 0, NS_NONE, [], None
        try:
            ids = self._ids_of(placement_names(fed))
        except O.ObjectError as e:
            err = str(e)
        if err is None and self.ftc.namespaced:  # computeNamespacedPlacement (placement.go:45-74)
            ns_name = _meta(fed).get("namespace", "")
            if ns_name in self.fed_namespaces:
                ns = self._namespace_row(ns_name)
                if ns < 0:
                    ns, err = NS_NONE, f"federated namespace {ns_name}: placement cannot be unmarshalled"
            else:
                ns = NS_NONE if self.limited_scope else NS_UNFEDERATED
        if err is not None:
            flags |= OBJ_ERROR
        behavior = orphaning_behavior(fed)
        flags |= OBJ_ORPHAN_ALL if behavior == ORPHAN_ALL else OBJ_ORPHAN_ADOPTED if behavior == ORPHAN_ADOPTED else 0
        obs = sorted((self.ids[n], observation_flags(m)) for n, m in member_objs.items() if n in self.ids and m is not None)
        self.obj_flags.append(flags)
        self.obj_ns.append(ns)
        self.pl_cluster += ids
        self.pl_off.append(len(self.pl_cluster))
        self.ob_cluster += [c for c, _ in obs]
        self.ob_flags += [f for _, f in obs]
        self.ob_off.append(len(self.ob_cluster))
        self.members.append(member_objs)
        self.errors.append(err)

    def arrays(self) -> dict:
        pl_off, ob_off = np.array(self.pl_off, np.int64), np.array(self.ob_off, np.int64)
        return {"cluster_flags": self.cluster_flags, "obj_flags": np.array(self.obj_flags, np.uint8),
                "obj_ns": np.array(self.obj_ns, np.int32), "obj_pl_off": pl_off.astype(np.int32),
                "pl_cluster": np.array(self.pl_cluster, np.int32), "ns_pl_off": np.array(self.ns_off, np.int32),
                "ns_cluster": np.array(self.ns_cluster, np.int32), "obj_ob_off": ob_off.astype(np.int32),
                "ob_cluster": np.array(self.ob_cluster, np.int32), "ob_flags": np.array(self.ob_flags, np.uint8),
                "out_off": pl_off + ob_off}  # the bound: a cluster neither selected nor observed emits nothing

    def selected_ids(self, k: int) -> Set[int]:
        """ComputePlacement of object k over the packed ids (the device reports its size as n_selected)."""
        if self.obj_flags[k] & OBJ_ERROR or self.obj_ns[k] == NS_UNFEDERATED:
            return set()
        sel = {c for c in self.pl_cluster[self.pl_off[k]:self.pl_off[k + 1]] if c >= 0}
        if self.obj_ns[k] >= 0:
            r = self.obj_ns[k]
            sel &= set(self.ns_cluster[self.ns_off[r]:self.ns_off[r + 1]])
        return sel

    def apply(self, result: dict) -> List[DispatchOutcome]:
        out = []
        out_off = np.array(self.pl_off, np.int64) + np.array(self.ob_off, np.int64)
        for k in range(len(self.obj_flags)):
            lo = int(out_off[k])
            hi = lo + int(result["count"][k])
            sel = self.selected_ids(k)
            if len(sel) != int(result["n_selected"][k]):
                raise RuntimeError(f"object {k}: kad_dispatch_plan selected {int(result['n_selected'][k])} clusters, the host {len(sel)}")
            ops, status = {}, {}
            for i in range(lo, hi):
                name = self.names[int(result["out_cluster"][i])]
                if result["out_op"][i] != OP_NONE:
                    ops[name] = int(result["out_op"][i])
                status[name] = STATUS_NAMES[int(result["out_status"][i])]
            res = int(result["obj_result"][k])
            members = {}
            for c, name in enumerate(self.names):
                m = self.members[k].get(name)
                if self.cluster_flags[c] & CL_READY and not isinstance(m, BaseException) and (c in sel or m is not None):
                    members[name] = m
            out.append(DispatchOutcome({self.names[c] for c in sel}, ops, status,
                                       {n for n, op in ops.items() if op in (OP_DELETE, OP_REMOVE_LABEL)},
                                       bool(res & RES_RECHECK), COMPUTE_PLACEMENT_FAILED if res & RES_PLACEMENT_FAILED else None,
                                       members))
        return out


def plan_numpy(cluster_flags, obj_flags, obj_ns, obj_pl_off, pl_cluster, ns_pl_off, ns_cluster, obj_ob_off, ob_cluster,
               ob_flags, out_off, fill: int = 0) -> dict:
    """kad_dispatch_plan's outputs, vectorised: the (object, cluster) pairs that are selected or observed as sorted
    keys object * C + cluster, the decision as a chain of masks over them, the emitted ones listed per object from
    out_off on. The slots behind an object's entries hold ``fill`` in every byte."""
    cf = np.asarray(cluster_flags, np.uint8).reshape(-1)
    of = np.asarray(obj_flags, np.uint8).reshape(-1)
    ns = np.asarray(obj_ns, np.int64).reshape(-1)
    C, n_obj = max(len(cf), 1), len(of)
    po, oo, fo = (np.asarray(a, np.int64).reshape(-1) for a in (obj_pl_off, obj_ob_off, out_off))
    no = np.asarray(ns_pl_off, np.int64).reshape(-1)
    pc, nc, oc = (np.asarray(a, np.int64).reshape(-1) for a in (pl_cluster, ns_cluster, ob_cluster))
    ob = np.asarray(ob_flags, np.uint8).reshape(-1)
    live = (of & OBJ_ERROR) == 0
    # the placement: union per object, without the names that are not joined, cut by the namespace row
    p_obj = np.repeat(np.arange(n_obj), np.diff(po))
    keep = (pc >= 0) & live[p_obj] & (ns[p_obj] != NS_UNFEDERATED)
    p_obj, p_cl = p_obj[keep], pc[keep]
    n_row = np.repeat(np.arange(len(no) - 1), np.diff(no))
    ns_keys = np.unique(n_row[nc >= 0] * C + nc[nc >= 0])
    in_ns = (ns[p_obj] < 0) | np.isin(np.maximum(ns[p_obj], 0) * C + p_cl, ns_keys)
    sel_keys = np.unique(p_obj[in_ns] * C + p_cl[in_ns])
    o_obj = np.repeat(np.arange(n_obj), np.diff(oo))
    ob_keys, ob_f = (o_obj * C + oc)[live[o_obj]], ob[live[o_obj]]
    keys = np.union1d(sel_keys, ob_keys)
    obj, cl = keys // C, keys % C
    sel = np.isin(keys, sel_keys)
    at = np.searchsorted(ob_keys, keys)
    seen = (at < len(ob_keys)) & (ob_keys[np.minimum(at, max(len(ob_keys) - 1, 0))] == keys) if len(ob_keys) else np.zeros(len(keys), bool)
    f = np.where(seen, ob_f[np.minimum(at, max(len(ob_f) - 1, 0))] if len(ob_f) else 0, 0).astype(np.uint8)
    c = cf[cl] if len(cf) else np.zeros(len(keys), np.uint8)
    ready, term, casc_ann, fin = ((c & b) != 0 for b in (CL_READY, CL_TERMINATING, CL_CASCADING, CL_FINALIZER))
    exists, deleting, adopted, failed = ((f & b) != 0 for b in (OB_EXISTS, OB_DELETING, OB_ADOPTED, OB_RETRIEVAL_FAILED))
    casc = term & casc_ann
    dele = ~sel | casc
    orphan = casc & (((of[obj] & OBJ_ORPHAN_ALL) != 0) | (((of[obj] & OBJ_ORPHAN_ADOPTED) != 0) & adopted))
    # the steps in the loop's order: the first that applies decides
    conds = [~ready, failed, dele & ~exists, dele & deleting, dele & term & ~casc_ann, dele & orphan, dele,
             term, ~fin, ~exists]
    ops = [OP_NONE, OP_NONE, OP_NONE, OP_NONE, OP_NONE, OP_REMOVE_LABEL, OP_DELETE, OP_NONE, OP_NONE, OP_CREATE]
    sts = [np.where(dele, ST_NONE, ST_CLUSTER_NOT_READY), ST_CACHED_RETRIEVAL_FAILED, ST_NONE, ST_WAITING_FOR_REMOVAL,
           ST_NONE, ST_LABEL_REMOVAL_TIMED_OUT, ST_DELETION_TIMED_OUT, ST_CLUSTER_TERMINATING,
           ST_FINALIZER_CHECK_FAILED, ST_CREATION_TIMED_OUT]
    op = np.select(conds, ops, OP_UPDATE)
    st = np.select(conds, sts, ST_UPDATE_TIMED_OUT)
    recheck = st == ST_FINALIZER_CHECK_FAILED
    emit = (op != OP_NONE) | (st != ST_NONE)
    e_obj = obj[emit]
    count = np.bincount(e_obj, minlength=n_obj).astype(np.int64)
    first = np.concatenate(([0], np.cumsum(count)))[:-1]
    pos = fo[e_obj] + (np.arange(len(e_obj)) - first[e_obj])
    cap = int(fo[-1]) if len(fo) else 0
    out_cluster = np.zeros(cap, np.int32)
    out_cluster.view(np.uint8)[:] = fill
    out_op, out_status = np.full(cap, fill, np.uint8), np.full(cap, fill, np.uint8)
    out_cluster[pos], out_op[pos], out_status[pos] = cl[emit], op[emit], st[emit]
    res = np.where(live, np.bincount(obj[recheck], minlength=n_obj) > 0, 0) * RES_RECHECK + ~live * RES_PLACEMENT_FAILED
    return {"out_cluster": out_cluster, "out_op": out_op, "out_status": out_status, "count": count.astype(np.int32),
            "n_ops": np.bincount(obj[op != OP_NONE], minlength=n_obj).astype(np.int32),
            "n_selected": np.bincount(sel_keys // C, minlength=n_obj).astype(np.int32), "obj_result": res.astype(np.uint8)}
