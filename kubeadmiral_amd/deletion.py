"""Sync deletion for a batch of federated objects: the host side of kad_deletion_plan and kad_deletion_finish.

The sync controller's reconcile has a second arm (pkg/controllers/sync/controller.go:340-378, 723-979): a federated
object with a deletion timestamp goes to ``ensureDeletion`` (orphan everything: ``removeManagedLabel``; otherwise
``deleteFromClusters`` and, once nothing remains, ``ensureRemovedOrUnmanaged``), and an event for a target without a
federated object goes to ``removeManagedLabel`` directly. This module restates everything around the two device calls:

* ``DeletionBatch`` — objects and the informers' member objects packed into the calls' arrays (the clusters' flags,
  the orphaning behaviour and the observations are dispatch.py's), the operations' and the checks' results packed for
  the second call, and both calls' outputs turned back into names, worker results and the reference's error texts
  (``apply_plan``, ``apply_finish``);
* ``plan_numpy`` / ``finish_numpy`` — both calls vectorised over the same arrays.

The operations and the GETs themselves, DeleteVersions, deleteHistory and the finalizer updates are the caller's.
"""

from __future__ import annotations

from typing import Dict, List, Optional, Sequence

import numpy as np

from . import dispatch as DI

FINALIZER_SYNC_CONTROLLER = DI.PREFIX + "sync-controller"
MANAGED_LABEL = DI.PREFIX + "managed"

# include/kad_sched.h
OBJ_HAS_FINALIZER, OBJ_ORPHAN_ALL, OBJ_ORPHAN_ADOPTED, OBJ_POSSIBLE_ORPHAN = 1, 2, 4, 8
PRE_RETRIEVAL_FAILED, PRE_NOT_READY = 1, 2
ACT_DELETE_HISTORY, ACT_REMOVE_FINALIZER, ACT_NOTHING, ACT_RECORD_ERROR = 1, 2, 4, 8
ACT_NAMES = ((ACT_DELETE_HISTORY, "delete-history"), (ACT_REMOVE_FINALIZER, "remove-finalizer"), (ACT_NOTHING, "nothing"),
             (ACT_RECORD_ERROR, "record-error"))
WAIT_TIMED_OUT, WAIT_CHECK_TIMED_OUT = 1, 2
CHK_GET_FAILED, CHK_DELETING, CHK_LABELLED, CHK_UNLABELLED = 1, 2, 4, 8
ST_OK, ST_ERROR, ST_RECHECK = range(3)
RESULT_NAMES = ("OK", "Error", "Recheck")  # worker.StatusAllOK, StatusError, Result{RequeueAfter: ensureDeletionRecheckDelay}
(RSN_NONE, RSN_TIMED_OUT, RSN_RETRIEVAL_FAILED, RSN_NOT_READY, RSN_OPS_FAILED, RSN_WAITING, RSN_CHECK_TIMED_OUT,
 RSN_CHECK_NOT_READY, RSN_CHECKS_FAILED) = range(9)
REASON_NAMES = ("", "TimedOut", "RetrievalFailed", "NotReady", "OpsFailed", "Waiting", "CheckTimedOut", "CheckNotReady",
                "ChecksFailed")
ENSURE_DELETION_FAILED = "EnsureDeletionFailed"
DISPATCH_TIMEOUT = "30s"  # operationDispatcherImpl.timeout (dispatch/operation.go:70) as %v prints it


def action_names(mask: int) -> List[str]:
    return [n for b, n in ACT_NAMES if mask & b]


class DeletionPlan:
    """One object before anything is sent: ``ops`` (cluster → dispatch.OP_DELETE / OP_REMOVE_LABEL, in joined-cluster
    order), ``remaining`` (deleteFromClusters' remainingClusters), ``retrieval_failed`` and ``unready`` (the names the
    two error strings of handleDeletionInClusters list; both empty where nothing is walked) and ``first`` (the actions
    that come before the operations)."""

    __slots__ = ("ops", "remaining", "retrieval_failed", "unready", "first")

    def __init__(self, ops, remaining, retrieval_failed, unready, first):
        self.ops, self.remaining, self.retrieval_failed, self.unready, self.first = ops, remaining, retrieval_failed, unready, first


class DeletionOutcome:
    """One object after Wait() and the live checks: ``result`` ("OK", "Error", "Recheck": the worker result), ``reason``
    (REASON_NAMES), ``error`` (the text of the error ensureDeletion or reconcile logs, None without one),
    ``recorded_error`` (the text ensureDeletion records as EnsureDeletionFailed, None where it records none) and ``then``
    (the actions that follow)."""

    __slots__ = ("result", "reason", "error", "recorded_error", "then")

    def __init__(self, result, reason, error, recorded_error, then):
        self.result, self.reason, self.error, self.recorded_error, self.then = result, reason, error, recorded_error, then


def _key(obj: Optional[dict]) -> str:
    md = DI._meta(obj)
    ns, name = md.get("namespace", "") or "", md.get("name", "") or ""
    return f"{ns}/{name}" if ns else name  # common.QualifiedName.String


class DeletionBatch:
    """Objects packed into kad_deletion_plan's and kad_deletion_finish's arrays. ``clusters``: the joined
    FederatedCluster objects as dicts, in the order that gives the cluster ids; ``finalizer``: the sync controller's
    cascading-delete finalizer on clusters (dispatch.cluster_flags_of reads it; the calls read the Ready bit only)."""

    def __init__(self, type_config, clusters: Sequence[dict], finalizer: str):
        self.ftc = type_config
        self.names = [DI._meta(c).get("name", "") for c in clusters]
        if len(self.names) > DI.MAX_CLUSTERS:
            raise ValueError(f"kad_deletion_plan covers at most {DI.MAX_CLUSTERS} joined clusters")
        self.ids = {n: i for i, n in enumerate(self.names)}
        self.finalizer = finalizer
        self.cluster_flags = np.array([DI.cluster_flags_of(c, finalizer) for c in clusters], np.uint8)
        self.obj_flags: List[int] = []
        self.ob_off, self.ob_cluster, self.ob_flags = [0], [], []
        self.feds: List[Optional[dict]] = []

    def __len__(self):
        return len(self.obj_flags)

    def add(self, fed: Optional[dict], member_objs: Dict[str, object]) -> None:
        """``fed``: the federated object (it has a deletion timestamp), or None where none exists (reconcile's
        possibleOrphan arm). ``member_objs``: per joined cluster name the informer's member object, None (or no key)
        where it holds none, or the exception the lookup failed with."""
        if fed is None:
            flags = OBJ_POSSIBLE_ORPHAN
        else:
            flags = OBJ_HAS_FINALIZER if FINALIZER_SYNC_CONTROLLER in (DI._meta(fed).get("finalizers") or []) else 0
            behavior = DI.orphaning_behavior(fed)
            flags |= OBJ_ORPHAN_ALL if behavior == DI.ORPHAN_ALL else OBJ_ORPHAN_ADOPTED if behavior == DI.ORPHAN_ADOPTED else 0
        obs = sorted((self.ids[n], DI.observation_flags(m)) for n, m in member_objs.items() if n in self.ids and m is not None)
        self.obj_flags.append(flags)
        self.ob_cluster += [c for c, _ in obs]
        self.ob_flags += [f for _, f in obs]
        self.ob_off.append(len(self.ob_cluster))
        self.feds.append(fed)

    def arrays(self) -> dict:
        return {"cluster_flags": self.cluster_flags, "obj_flags": np.array(self.obj_flags, np.uint8),
                "obj_ob_off": np.array(self.ob_off, np.int32), "ob_cluster": np.array(self.ob_cluster, np.int32),
                "ob_flags": np.array(self.ob_flags, np.uint8)}

    def finish_arrays(self, op_results: Sequence[Dict[str, bool]], waits: Optional[Sequence[int]] = None,
                      checks: Optional[Sequence[Dict[str, object]]] = None,
                      check_clusters: Optional[Sequence[dict]] = None) -> dict:
        """``op_results[k]``: per cluster whether object k's operation succeeded (a cluster without a key: it did);
        ``waits[k]``: WAIT_* bits; ``checks[k]``: per cluster what ensureRemovedOrUnmanaged's GET answered, other than
        NotFound: the member object, or the exception it failed with; ``check_clusters``: the joined clusters as listed
        the second time (the same names in the same order; default: unchanged)."""
        a = self.arrays()
        n = len(self)
        ok = np.ones(len(self.ob_cluster), np.uint8)
        for k, res in enumerate(op_results):
            for i in range(self.ob_off[k], self.ob_off[k + 1]):
                if not res.get(self.names[self.ob_cluster[i]], True):
                    ok[i] = 0
        off, cl, fl = [0], [], []
        for k in range(n):
            rows = []
            for name, m in ((checks[k] if checks else None) or {}).items():
                if name not in self.ids or m is None:
                    continue
                if isinstance(m, BaseException):
                    f = CHK_GET_FAILED
                elif DI._meta(m).get("deletionTimestamp") is not None:
                    f = CHK_DELETING
                else:
                    labels = DI._meta(m).get("labels")
                    f = CHK_LABELLED if isinstance(labels, dict) and labels.get(MANAGED_LABEL) == "true" else CHK_UNLABELLED
                rows.append((self.ids[name], f))
            rows.sort()
            cl += [c for c, _ in rows]
            fl += [f for _, f in rows]
            off.append(len(cl))
        if check_clusters is None:
            ccf = self.cluster_flags
        else:
            if [DI._meta(c).get("name", "") for c in check_clusters] != self.names:
                raise ValueError("check_clusters: not the batch's joined clusters in their order")
            ccf = np.array([DI.cluster_flags_of(c, self.finalizer) for c in check_clusters], np.uint8)
        a.update(op_ok=ok, obj_wait=np.array(list(waits) if waits is not None else [0] * n, np.uint8),
                 chk_off=np.array(off, np.int32), chk_cluster=np.array(cl, np.int32), chk_flags=np.array(fl, np.uint8),
                 chk_cluster_flags=ccf)
        return a

    def _unready(self, flags) -> List[str]:
        return [n for n, f in zip(self.names, flags) if not f & DI.CL_READY]

    def apply_plan(self, result: dict) -> List[DeletionPlan]:
        out = []
        unready = self._unready(self.cluster_flags)
        for k, of in enumerate(self.obj_flags):
            lo, hi = self.ob_off[k], self.ob_off[k + 1]
            walks = bool(of & (OBJ_HAS_FINALIZER | OBJ_POSSIBLE_ORPHAN))
            label_arm = bool(of & (OBJ_ORPHAN_ALL | OBJ_POSSIBLE_ORPHAN))
            ops, remaining, failed = {}, [], []
            for i in range(lo, hi):
                c, f = self.ob_cluster[i], self.ob_flags[i]
                name, op = self.names[c], int(result["out_op"][i])
                if op != DI.OP_NONE:
                    ops[name] = op
                if walks and self.cluster_flags[c] & DI.CL_READY:
                    if f & DI.OB_RETRIEVAL_FAILED:
                        failed.append(name)
                    elif not label_arm:
                        remaining.append(name)
            if (len(ops), len(remaining), len(failed)) != (int(result["n_ops"][k]), int(result["n_remaining"][k]),
                                                           int(result["n_retrieval_failed"][k])):
                raise RuntimeError(f"object {k}: kad_deletion_plan's counts differ from its operations and the host's lists")
            pre = int(result["obj_pre"][k])
            if bool(pre & PRE_NOT_READY) != bool(walks and unready) or bool(pre & PRE_RETRIEVAL_FAILED) != bool(failed):
                raise RuntimeError(f"object {k}: kad_deletion_plan's obj_pre differs from the host's lists")
            out.append(DeletionPlan(ops, remaining, failed, unready if walks else [], action_names(int(result["obj_first"][k]))))
        return out

    def apply_finish(self, result: dict, plans: Sequence[DeletionPlan], check_clusters: Optional[Sequence[dict]] = None) -> List[DeletionOutcome]:
        """``plans``: :meth:`apply_plan`'s of the same batch (the names the error texts list)."""
        unready2 = self._unready(self.cluster_flags if check_clusters is None
                                 else [DI.cluster_flags_of(c, self.finalizer) for c in check_clusters])
        n_checks = len(self.names) - len(unready2)
        out = []
        for k, (of, p) in enumerate(zip(self.obj_flags, plans)):
            reason = int(result["obj_reason"][k])
            label_arm = bool(of & (OBJ_ORPHAN_ALL | OBJ_POSSIBLE_ORPHAN))
            err = {
                RSN_TIMED_OUT: f"Failed to finish {len(p.ops)} operations in {DISPATCH_TIMEOUT}",
                RSN_RETRIEVAL_FAILED: "failed to retrieve a managed resource for the following cluster(s): " + ", ".join(p.retrieval_failed),
                RSN_NOT_READY: "the following clusters were not ready: " + ", ".join(p.unready),
                RSN_OPS_FAILED: ("failed to remove the label from resources in one or more clusters." if label_arm
                                 else "failed to remove managed resources from one or more clusters."),
                RSN_CHECK_TIMED_OUT: f"Failed to finish {n_checks} operations in {DISPATCH_TIMEOUT}",
                RSN_CHECK_NOT_READY: "the following clusters were not ready: " + ", ".join(unready2),
                RSN_CHECKS_FAILED: "one or more checks failed",
            }.get(reason)
            if reason >= RSN_CHECK_TIMED_OUT:
                err = "failed to verify that managed resources no longer exist in any cluster: " + err
            then = int(result["obj_then"][k])
            recorded = None
            if then & ACT_RECORD_ERROR:
                fed = self.feds[k]
                recorded = f"failed to delete {(fed or {}).get('kind', '')} \"{_key(fed)}\": {err}"
            out.append(DeletionOutcome(RESULT_NAMES[int(result["obj_status"][k])], REASON_NAMES[reason], err, recorded,
                                       action_names(then)))
        return out


def _walk(cluster_flags, obj_flags, obj_ob_off, ob_cluster, ob_flags):
    cf = np.asarray(cluster_flags, np.uint8).reshape(-1)
    of = np.asarray(obj_flags, np.uint8).reshape(-1)
    oo = np.asarray(obj_ob_off, np.int64).reshape(-1)
    oc = np.asarray(ob_cluster, np.int64).reshape(-1)
    ob = np.asarray(ob_flags, np.uint8).reshape(-1)
    n = len(of)
    owner = np.repeat(np.arange(n), np.diff(oo))
    walks = (of & (OBJ_HAS_FINALIZER | OBJ_POSSIBLE_ORPHAN)) != 0
    label_arm = (of & (OBJ_ORPHAN_ALL | OBJ_POSSIBLE_ORPHAN)) != 0
    live = walks[owner] & ((cf[oc] & DI.CL_READY) != 0) if len(oc) else np.zeros(0, bool)
    failed = live & ((ob & DI.OB_RETRIEVAL_FAILED) != 0)
    exists = live & ((ob & DI.OB_EXISTS) != 0)
    la = label_arm[owner]
    remaining = exists & ~la
    orphan = ((of[owner] & OBJ_ORPHAN_ADOPTED) != 0) & ((ob & DI.OB_ADOPTED) != 0)
    op = np.where(exists & la & ((ob & DI.OB_DELETING) == 0), DI.OP_REMOVE_LABEL,
                  np.where(remaining, np.where(orphan, DI.OP_REMOVE_LABEL, DI.OP_DELETE), DI.OP_NONE)).astype(np.uint8)
    count = lambda m: np.bincount(owner[m], minlength=n).astype(np.int32)  # noqa: E731
    return cf, of, owner, walks, label_arm, op, count(op != DI.OP_NONE), count(remaining), count(failed)


def plan_numpy(cluster_flags, obj_flags, obj_ob_off, ob_cluster, ob_flags) -> dict:
    """kad_deletion_plan's outputs, vectorised over the observations."""
    cf, of, _, walks, _, op, n_ops, n_rem, n_rf = _walk(cluster_flags, obj_flags, obj_ob_off, ob_cluster, ob_flags)
    unready = int(((cf & DI.CL_READY) == 0).sum())
    pre = np.where(walks, (n_rf > 0) * PRE_RETRIEVAL_FAILED + (unready > 0) * PRE_NOT_READY, 0).astype(np.uint8)
    orphan_all = walks & ((of & OBJ_ORPHAN_ALL) != 0) & ((of & OBJ_POSSIBLE_ORPHAN) == 0)
    first = np.where(walks, orphan_all * (ACT_DELETE_HISTORY | ACT_REMOVE_FINALIZER), ACT_NOTHING).astype(np.uint8)
    return {"out_op": op, "n_ops": n_ops, "n_remaining": n_rem, "n_retrieval_failed": n_rf, "obj_pre": pre, "obj_first": first}


def finish_numpy(cluster_flags, obj_flags, obj_ob_off, ob_cluster, ob_flags, op_ok, obj_wait, chk_off, chk_cluster, chk_flags,
                 chk_cluster_flags) -> dict:
    """kad_deletion_finish's outputs, vectorised: the reasons as a chain of masks in the reference's order."""
    cf, of, owner, walks, label_arm, op, n_ops, n_rem, n_rf = _walk(cluster_flags, obj_flags, obj_ob_off, ob_cluster, ob_flags)
    n = len(of)
    ok = np.asarray(op_ok, np.uint8).reshape(-1)
    wait = np.asarray(obj_wait, np.uint8).reshape(-1)
    n_fail = np.bincount(owner[(op != DI.OP_NONE) & (ok == 0)], minlength=n).astype(np.int32)
    ccf = np.asarray(chk_cluster_flags, np.uint8).reshape(-1)
    ko = np.asarray(chk_off, np.int64).reshape(-1)
    kc = np.asarray(chk_cluster, np.int64).reshape(-1)
    kf = np.asarray(chk_flags, np.uint8).reshape(-1)
    k_owner = np.repeat(np.arange(n), np.diff(ko))
    k_bad = ((ccf[kc] & DI.CL_READY) != 0) & (kf != CHK_UNLABELLED) if len(kc) else np.zeros(0, bool)
    n_fc = np.bincount(k_owner[k_bad], minlength=n).astype(np.int32)
    unready = int(((cf & DI.CL_READY) == 0).sum())
    unready2 = int(((ccf & DI.CL_READY) == 0).sum())
    first = [((wait & WAIT_TIMED_OUT) != 0) & (n_ops > 0), n_rf > 0, np.full(n, unready > 0), n_fail > 0]
    reason1 = np.select(first, [RSN_TIMED_OUT, RSN_RETRIEVAL_FAILED, RSN_NOT_READY, RSN_OPS_FAILED], RSN_NONE)
    reason1 = np.where(walks, reason1, RSN_NONE)
    delete_arm = walks & ~label_arm
    waiting = delete_arm & (reason1 == RSN_NONE) & (n_rem > 0)
    checked = delete_arm & (reason1 == RSN_NONE) & (n_rem == 0)
    second = [((wait & WAIT_CHECK_TIMED_OUT) != 0) & (unready2 < len(ccf)), np.full(n, unready2 > 0), n_fc > 0]
    reason2 = np.select(second, [RSN_CHECK_TIMED_OUT, RSN_CHECK_NOT_READY, RSN_CHECKS_FAILED], RSN_NONE)
    reason = np.where(reason1 != RSN_NONE, reason1, np.where(waiting, RSN_WAITING, np.where(checked, reason2, RSN_NONE)))
    error = (reason != RSN_NONE) & (reason != RSN_WAITING)
    status = np.where(error, ST_ERROR, np.where(waiting, ST_RECHECK, ST_OK))
    then = np.where(error & delete_arm, ACT_RECORD_ERROR,
                    np.where(checked & ~error, ACT_DELETE_HISTORY | ACT_REMOVE_FINALIZER, 0))
    return {"obj_status": status.astype(np.uint8), "obj_reason": reason.astype(np.uint8), "obj_then": then.astype(np.uint8),
            "n_failed_ops": np.where(walks, n_fail, 0).astype(np.int32), "n_failed_checks": np.where(checked, n_fc, 0).astype(np.int32)}
