"""Sync completion for a batch of federated objects: the host side of kad_sync_needs_update and kad_sync_finish.

After ``reconcile_dispatch`` has decided the operations, the sync controller checks every update against the
propagated versions and, once ``dispatcher.Wait()`` returns, closes the reconcile (syncToClusters,
pkg/controllers/sync/controller.go:546-596). This module restates everything around the two device calls:

* ``object_version`` / ``generation_of_version`` — ObjectVersion and the strconv.ParseInt rule of
  ConvertVersionMapToGenerationMap (util/propagatedversion.go:43-49, 138-157);
* ``needs_update_flags`` — the field reads of ObjectNeedsUpdate (propagatedversion.go:65-118) with
  ``object_meta_equivalent`` (ObjectMetaObjEquivalent, util/meta.go:90-108);
* ``PropagatedVersions`` — the VersionManager's state without the API (sync/version/manager.go);
* ``SyncFinishBatch`` — version strings and reasons interned, clusters ordered by name, stored lists normalised,
  the arrays of both calls, and their outputs turned back into names, version objects and statuses (``apply``);
* ``needs_update_numpy`` / ``finish_numpy`` — both calls vectorised over the same arrays.

The operations themselves and the API writes stay with the caller.
"""

from __future__ import annotations

import re
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

from .rollout import MAX_SURGE_FIELDS, MAX_UNAVAILABLE_FIELDS, RolloutError, _is_int, _nested, nested_int64, split_dot_path

# kad_sync_*'s constants (include/kad_sched.h); the statuses in the order of types_status.go:71-99
MAX_CLUSTERS = 16384
STATUS_NAMES = ("", "OK", "WaitingForRemoval", "ClusterNotReady", "ClusterTerminating", "CachedRetrievalFailed",
                "ComputeResourceFailed", "ApplyOverridesFailed", "CreationFailed", "UpdateFailed", "DeletionFailed",
                "LabelRemovalFailed", "RetrievalFailed", "AlreadyExists", "FieldRetentionFailed",
                "SetLastReplicasetNameFailed", "VersionRetrievalFailed", "ClientRetrievalFailed", "ManagedLabelFalse",
                "FinalizerCheckFailed", "CreationTimedOut", "UpdateTimedOut", "DeletionTimedOut", "LabelRemovalTimedOut")
STATUS_CODE = {n: i for i, n in enumerate(STATUS_NAMES)}
ST_OK, ST_WAITING_FOR_REMOVAL = 1, 2
ST_CREATION_TIMED_OUT, ST_UPDATE_TIMED_OUT, ST_DELETION_TIMED_OUT, ST_LABEL_REMOVAL_TIMED_OUT, ST_MAX = 20, 21, 22, 23, 23
VER_HAS_GEN, VER_IS_GEN = 1, 2
ROW_REPLICAS_EQUAL, ROW_SURGE_EQUAL, ROW_UNAVAILABLE_EQUAL, ROW_META_EQUIVALENT = 1, 2, 4, 8
(OBJ_VERSION_EXISTS, OBJ_VERSIONS_CURRENT, OBJ_OLDV_NIL, OBJ_OLDV_IRREGULAR, OBJ_RESOURCES_UPDATED, OBJ_SCALARS_CHANGED,
 OBJ_COND_EXISTS, OBJ_COND_TRUE, OBJ_STATUS_ON_HOST) = (1 << i for i in range(9))
OUT_CLUSTERS_CHANGED, OUT_CHANGES_PROPAGATED, OUT_TRANSITION, OUT_UPDATE_REQUIRED, OUT_STATUS_WRITE = 1, 2, 4, 8, 16
AGGREGATE_SUCCESS, CHECK_CLUSTERS, NAMESPACE_NOT_FEDERATED = "", "CheckClusters", "NamespaceNotFederated"
REASON_CHECK_CLUSTERS, REASON_NS_NOT_FEDERATED = 1, 2  # their ids in every batch
PROPAGATION_CONDITION = "Propagation"
GENERATION_PREFIX, RESOURCE_VERSION_PREFIX = "gen:", "rv:"
_TRANSITION = np.arange(ST_MAX + 1, dtype=np.uint8)  # Wait() (managed.go:137-155)
_TRANSITION[[ST_CREATION_TIMED_OUT, ST_UPDATE_TIMED_OUT]] = ST_OK
_TRANSITION[ST_DELETION_TIMED_OUT] = ST_WAITING_FOR_REMOVAL
_TRANSITION[ST_LABEL_REMOVAL_TIMED_OUT] = 0
_INT = re.compile(r"[+-]?[0-9]+\Z")


def _meta(obj) -> dict:
    m = obj.get("metadata") if isinstance(obj, dict) else None
    return m if isinstance(m, dict) else {}


def object_version(member: dict) -> str:
    """ObjectVersion (propagatedversion.go:43-49): the generation where the object has one, else the resource
    version."""
    g = _meta(member).get("generation")
    if _is_int(g) and g != 0:
        return f"{GENERATION_PREFIX}{g}"
    rv = _meta(member).get("resourceVersion")
    return RESOURCE_VERSION_PREFIX + (rv if isinstance(rv, str) else "")


def generation_of_version(version: str) -> Optional[int]:
    """The entry ConvertVersionMapToGenerationMap makes of a version string (propagatedversion.go:140-155): 0 for
    an ``rv:`` prefix, the number behind ``gen:`` where strconv.ParseInt(s, 10, 64) accepts it (a sign, decimal
    digits, within int64), else None."""
    if version.startswith(RESOURCE_VERSION_PREFIX):
        return 0
    if not version.startswith(GENERATION_PREFIX):
        return None
    s = version[len(GENERATION_PREFIX):]
    if not _INT.match(s) or not s.isascii():
        return None
    g = int(s)
    return g if -2 ** 63 <= g < 2 ** 63 else None


def version_flags(version: str) -> Tuple[int, int]:
    """(ver_flags, ver_gen) of one version string."""
    g = generation_of_version(version)
    return (0 if g is None else VER_HAS_GEN) | (VER_IS_GEN if version.startswith(GENERATION_PREFIX) else 0), g or 0


def _string_map(obj, key: str) -> dict:
    """GetLabels / GetAnnotations: NestedStringMap, nil where it errs."""
    m = _meta(obj).get(key)
    return dict(m) if isinstance(m, dict) and all(isinstance(v, str) for v in m.values()) else {}


def _meta_string(obj, key: str) -> str:
    v = _meta(obj).get(key)
    return v if isinstance(v, str) else ""


def object_meta_equivalent(a: dict, b: dict) -> bool:
    """ObjectMetaObjEquivalent (util/meta.go:90-108): name, namespace, labels and annotations; a nil map and an
    empty one are equivalent (:99, :104)."""
    return (_meta_string(a, "name") == _meta_string(b, "name") and _meta_string(a, "namespace") == _meta_string(b, "namespace")
            and _string_map(a, "labels") == _string_map(b, "labels")
            and _string_map(a, "annotations") == _string_map(b, "annotations"))


def _nested_string(obj: dict, fields) -> Tuple[str, bool]:
    """unstructured.NestedString: ("", False) when absent, an error for another type."""
    v, found = _nested(obj, fields)
    if not found:
        return "", False
    if not isinstance(v, str):
        raise RolloutError(f"{'.'.join(fields)} accessor error: {v!r} is not a string")
    return v, True


def _nested_int(obj: dict, fields) -> Tuple[int, bool]:
    v = nested_int64(obj, fields)
    return (0, False) if v is None else (v, True)


def _int_or_string_equal(desired: dict, member: dict, fields) -> bool:
    """propagatedversion.go:78-92 (and :97-111): the int64 branch is reached only when the string read of the
    desired object errs; ok == ok2 is required."""
    try:
        d, ok = _nested_string(desired, fields)
    except RolloutError:
        try:
            di, ok = _nested_int(desired, fields)
            ci, ok2 = _nested_int(member, fields)
        except RolloutError:
            return False
        return ok == ok2 and di == ci
    try:
        c, ok2 = _nested_string(member, fields)
    except RolloutError:
        return False
    return ok == ok2 and d == c


def needs_update_flags(desired: dict, member: dict, replicas_spec: str) -> int:
    """The KAD_SYNC_ROW_* flags of one update: what ObjectNeedsUpdate reads from the desired and the member
    object. nil and nil replicas compare equal (propagatedversion.go:68); a read that errs leaves the flag clear,
    as an empty replicas path does (NestedInt64 then meets the object itself)."""
    f = 0
    fields = split_dot_path(replicas_spec)
    try:
        if nested_int64(desired, fields) == nested_int64(member, fields):
            f |= ROW_REPLICAS_EQUAL
    except RolloutError:
        pass
    if _int_or_string_equal(desired, member, MAX_SURGE_FIELDS):
        f |= ROW_SURGE_EQUAL
    if _int_or_string_equal(desired, member, MAX_UNAVAILABLE_FIELDS):
        f |= ROW_UNAVAILABLE_EQUAL
    if object_meta_equivalent(desired, member):
        f |= ROW_META_EQUIVALENT
    return f


def propagated_version_name(kind: str, name: str) -> str:
    """PropagatedVersionName (manager.go:481-487)."""
    return f"{kind.lower()}-{name}"


class PropagatedVersions:
    """The VersionManager's in-memory state without the API: the PropagatedVersion objects of one target kind by
    (namespace, version object name)."""

    def __init__(self, target_kind: str):
        self.kind = target_kind
        self.versions: Dict[Tuple[str, str], dict] = {}

    def key(self, namespace: str, name: str) -> Tuple[str, str]:
        return namespace or "", propagated_version_name(self.kind, name)

    def status(self, namespace: str, name: str) -> Optional[dict]:
        obj = self.versions.get(self.key(namespace, name))
        return None if obj is None else (obj.get("status") or {})

    def get(self, namespace: str, name: str, template_version: str, override_version: str) -> Dict[str, str]:
        """VersionManager.Get (manager.go:119-148)."""
        st = self.status(namespace, name)
        if st is None or st.get("templateVersion", "") != template_version or st.get("overrideVersion", "") != override_version:
            return {}
        out = {}
        for cv in st.get("clusterVersions") or []:
            out[cv.get("clusterName", "")] = cv.get("version", "")
        return out

    def set_status(self, namespace: str, name: str, status: dict) -> dict:
        """The in-memory half of Update (manager.go:196-202); writing the object is the caller's."""
        ns, vname = self.key(namespace, name)
        obj = self.versions.setdefault((ns, vname), {"metadata": {"name": vname, **({"namespace": ns} if ns else {})}})
        obj["status"] = status
        return obj

    def delete(self, namespace: str, name: str) -> None:
        self.versions.pop(self.key(namespace, name), None)


class FinishOutcome:
    """One object's answer: ``version_status`` (the new PropagatedVersion status) and ``version_write``;
    ``status`` (the object's new status) and ``status_write`` (UpdateStatus is due); ``reason`` (the aggregate
    reason of the propagation condition) and ``clusters_changed``."""

    __slots__ = ("version_status", "version_write", "status", "status_write", "reason", "clusters_changed")

    def __init__(self, version_status, version_write, status, status_write, reason, clusters_changed):
        self.version_status, self.version_write, self.status = version_status, version_write, status
        self.status_write, self.reason, self.clusters_changed = status_write, reason, clusters_changed


def _csr(rows: Sequence[Sequence], dtype=np.int32):
    off = np.zeros(len(rows) + 1, np.int64)
    np.cumsum([len(r) for r in rows], out=off[1:])
    flat = np.array([x for r in rows for x in r], dtype) if off[-1] else np.zeros(0, dtype)
    return off, flat


class SyncFinishBatch:
    """Objects packed into the arrays of kad_sync_needs_update (``add_versions`` / ``add_update``) and
    kad_sync_finish (``add``). ``cluster_names``: the joined clusters; ids follow the ascending byte order of the
    names, whatever order they come in."""

    def __init__(self, cluster_names: Sequence[str]):
        self.names = sorted(set(cluster_names), key=lambda n: n.encode())
        if len(self.names) > MAX_CLUSTERS:
            raise ValueError(f"kad_sync_finish covers at most {MAX_CLUSTERS} joined clusters")
        self.ids = {n: i for i, n in enumerate(self.names)}
        self.versions, self.ver_ids = [""], {"": 0}
        self.reasons = [AGGREGATE_SUCCESS, CHECK_CLUSTERS, NAMESPACE_NOT_FEDERATED]
        self.reason_ids = {r: i for i, r in enumerate(self.reasons)}
        # needs-update half
        self.nu_obj_flags, self.nu_rec, self.rows = [], [], []
        # finish half
        self.objs: List[dict] = []

    def version_id(self, version: str) -> int:
        if version not in self.ver_ids:
            self.ver_ids[version] = len(self.versions)
            self.versions.append(version)
        return self.ver_ids[version]

    def reason_id(self, reason: str) -> int:
        if reason not in self.reason_ids:
            self.reason_ids[reason] = len(self.reasons)
            self.reasons.append(reason)
        return self.reason_ids[reason]

    def _version_table(self):
        fl = [version_flags(v) for v in self.versions]
        return np.array([f for f, _ in fl], np.uint8), np.array([g for _, g in fl], np.int64)

    @staticmethod
    def _current(stored: Optional[dict], template_version: str, override_version: str) -> bool:
        return (stored is not None and stored.get("templateVersion", "") == template_version
                and stored.get("overrideVersion", "") == override_version)

    def _normalise_versions(self, stored: Optional[dict]):
        """The stored clusterVersions as ascending (cluster id, version id) → (list, nil, irregular). An unknown
        cluster, a duplicate (the first is kept, as updateClusterVersions keeps it), an empty version (never part of
        a new list) or a list out of order makes it irregular."""
        raw = None if stored is None else stored.get("clusterVersions")
        if raw is None:
            return [], stored is not None, False
        seen, out, irregular = set(), [], False
        for cv in raw:
            c = self.ids.get(cv.get("clusterName", ""))
            v = cv.get("version", "")
            if c is None or c in seen or v == "":
                irregular = True
                continue
            seen.add(c)
            out.append((c, self.version_id(v)))
        if any(out[i][0] > out[i + 1][0] for i in range(len(out) - 1)):
            irregular = True
            out.sort()
        return out, False, irregular

    # ------------------------------------------------------------------ the version check
    def add_versions(self, stored: Optional[dict], template_version: str, override_version: str) -> int:
        """One object of the needs-update half: its stored PropagatedVersion status (None: none stored) and its
        template and override versions → the object's index for :meth:`add_update`."""
        cur = self._current(stored, template_version, override_version)
        rec = []
        if cur:  # VersionManager.Get (manager.go:142-144): a map, so a later duplicate wins
            last = {}
            for cv in stored.get("clusterVersions") or []:
                c = self.ids.get(cv.get("clusterName", ""))
                if c is not None:
                    last[c] = self.version_id(cv.get("version", ""))
            rec = sorted(last.items())
        self.nu_obj_flags.append(1 if cur else 0)
        self.nu_rec.append(rec)
        return len(self.nu_obj_flags) - 1

    def add_update(self, obj_index: int, cluster: str, desired: dict, member: dict, replicas_spec: str) -> None:
        """One update: the object :meth:`add_versions` returned, the member cluster, the object to be written and the
        member cluster's current one."""
        self.rows.append((obj_index, self.ids[cluster], self.version_id(object_version(member)),
                          needs_update_flags(desired, member, replicas_spec)))

    def needs_update_arrays(self) -> dict:
        off, _ = _csr(self.nu_rec)
        vf, _ = self._version_table()
        col = lambda k, dt: np.array([r[k] for r in self.rows], dt)  # noqa: E731
        return {"n_clusters": len(self.names), "row_obj": col(0, np.int32), "row_cluster": col(1, np.int32),
                "row_target": col(2, np.int32), "row_flags": col(3, np.uint8),
                "obj_flags": np.array(self.nu_obj_flags, np.uint8), "rec_off": off.astype(np.int32),
                "rec_cluster": np.array([c for r in self.nu_rec for c, _ in r], np.int32),
                "rec_version": np.array([v for r in self.nu_rec for _, v in r], np.int32), "ver_flags": vf}

    def apply_needs_update(self, result: dict) -> List[Dict[str, Tuple[bool, str]]]:
        """Per object: cluster → (the member object needs the update, the version VersionForCluster returned)."""
        out: List[Dict[str, Tuple[bool, str]]] = [{} for _ in self.nu_obj_flags]
        for (o, c, _, _), need, rec in zip(self.rows, result["needs_update"], result["recorded"]):
            out[o][self.names[c]] = (bool(need), self.versions[int(rec)])
        return out

    # ------------------------------------------------------------------ the close of the reconcile
    def add(self, status: Optional[dict], generation: int, collision_count: Optional[int], selected: Sequence[str],
            records: Dict[str, Tuple[str, str]], resources_updated: bool, stored_version: Optional[dict],
            template_version: str, override_version: str, reason: str = AGGREGATE_SUCCESS,
            namespace_not_federated: bool = False) -> None:
        """One object whose Wait() did not time out. ``status``: the federated object's stored status (None: none);
        ``generation`` / ``collision_count``: what update compares syncedGeneration and collisionCount with;
        ``selected``: the placement; ``records``: cluster → (the status the dispatcher holds when the operations have
        ended, before Wait's transitions; the version recordVersion recorded, or ""); ``stored_version``: the stored
        PropagatedVersion status (None: none); ``reason`` as syncToClusters passes it, with NamespaceNotFederated
        applied here (controller.go:649-656)."""
        status = status if isinstance(status, dict) else {}
        if reason == AGGREGATE_SUCCESS and namespace_not_federated:
            reason = NAMESPACE_NOT_FEDERATED
        flags = 0
        cur = self._current(stored_version, template_version, override_version)
        oldv, nil, irregular = self._normalise_versions(stored_version)
        flags |= (OBJ_VERSION_EXISTS if stored_version is not None else 0) | (OBJ_VERSIONS_CURRENT if cur else 0)
        flags |= (OBJ_OLDV_NIL if nil else 0) | (OBJ_OLDV_IRREGULAR if irregular else 0)
        flags |= OBJ_RESOURCES_UPDATED if resources_updated else 0
        if status.get("syncedGeneration", 0) != generation or status.get("collisionCount") != collision_count:
            flags |= OBJ_SCALARS_CHANGED
        cond = next((c for c in status.get("conditions") or [] if isinstance(c, dict) and c.get("type") == PROPAGATION_CONDITION), None)
        cond_reason = 0
        if cond is not None:
            flags |= OBJ_COND_EXISTS | (OBJ_COND_TRUE if cond.get("status") == "True" else 0)
            cond_reason = self.reason_id(cond.get("reason", "")) if cond.get("status") in ("True", "False") else -1
        olds, on_host, seen = [], False, set()
        for cl in status.get("clusters") or []:
            c, s = self.ids.get(cl.get("name", "")), STATUS_CODE.get(cl.get("status", ""), 0)
            if c is None or c in seen or s == 0:
                on_host = True
                break
            seen.add(c)
            olds.append((c, s, int(cl.get("generation", 0))))
        if on_host:
            flags |= OBJ_STATUS_ON_HOST
            olds = []
        ent = sorted((self.ids[n], STATUS_CODE[s], self.version_id(v)) for n, (s, v) in records.items())
        self.objs.append({"flags": flags, "reason_in": self.reason_id(reason), "cond_reason": cond_reason,
                          "sel": sorted({self.ids[n] for n in selected if n in self.ids}), "ent": ent, "oldv": oldv,
                          "olds": sorted(olds), "status": status, "generation": generation, "collision": collision_count,
                          "records": records, "resources_updated": resources_updated, "reason": reason,
                          "template": template_version, "override": override_version})

    def __len__(self):
        return len(self.objs)

    def finish_arrays(self) -> dict:
        o = self.objs
        lists = {k: np.concatenate(([0], np.cumsum([len(x[k]) for x in o]))).astype(np.int64) for k in ("sel", "ent", "oldv", "olds")}
        col = lambda k, i, dt: np.array([e[i] for x in o for e in x[k]], dt)  # noqa: E731
        vf, vg = self._version_table()
        ne, nv = np.diff(lists["ent"]), np.diff(lists["oldv"])
        return {"n_clusters": len(self.names), "n_reasons": len(self.reasons), "reason_check_clusters": REASON_CHECK_CLUSTERS,
                "reason_ns_not_federated": REASON_NS_NOT_FEDERATED,
                "obj_flags": np.array([x["flags"] for x in o], np.uint16),
                "reason_in": np.array([x["reason_in"] for x in o], np.int32),
                "cond_reason": np.array([x["cond_reason"] for x in o], np.int32),
                "sel_off": lists["sel"].astype(np.int32), "sel_cluster": np.array([c for x in o for c in x["sel"]], np.int32),
                "ent_off": lists["ent"].astype(np.int32), "ent_cluster": col("ent", 0, np.int32),
                "ent_status": col("ent", 1, np.uint8), "ent_version": col("ent", 2, np.int32),
                "oldv_off": lists["oldv"].astype(np.int32), "oldv_cluster": col("oldv", 0, np.int32),
                "oldv_version": col("oldv", 1, np.int32),
                "olds_off": lists["olds"].astype(np.int32), "olds_cluster": col("olds", 0, np.int32),
                "olds_status": col("olds", 1, np.uint8), "olds_gen": col("olds", 2, np.int64),
                "ver_gen": vg, "ver_flags": vf,
                "ver_off": np.concatenate(([0], np.cumsum(ne + nv))).astype(np.int64),
                "st_off": np.concatenate(([0], np.cumsum(ne))).astype(np.int64)}

    def _status_on_host(self, x: dict) -> Tuple[int, str, List[dict]]:
        """status.update's decisions for one object with Go's maps, for a stored status.clusters that is irregular
        (status.go:104-120, 159-179) → (obj_out bits, the reason, status.clusters)."""
        status_map, gen_map = {}, {}
        for name, (s, v) in x["records"].items():
            s2 = STATUS_NAMES[int(_TRANSITION[STATUS_CODE[s]])]
            if s2:
                status_map[name] = s2
            g = generation_of_version(v) if v else None
            if g is not None:
                gen_map[name] = g
        reason = x["reason"]
        if reason == AGGREGATE_SUCCESS and any(s != "OK" for s in status_map.values()):
            reason = CHECK_CLUSTERS
        old = x["status"].get("clusters") or []
        differs = len(old) != len(status_map) or len(old) != len(gen_map) or any(
            status_map.get(c.get("name", ""), "") != c.get("status", "") or gen_map.get(c.get("name", ""), 0) != c.get("generation", 0)
            for c in old)
        clusters = [{"name": n, "status": status_map[n], **({"generation": gen_map[n]} if gen_map.get(n, 0) else {})}
                    for n in sorted(status_map, key=lambda n: n.encode())]
        return self._decide(x["flags"], differs, bool(status_map), reason, x["cond_reason"]), reason, clusters

    def _decide(self, flags: int, differs: bool, has_status: bool, reason: str, cond_reason: int) -> int:
        propagated = differs or (has_status and bool(flags & OBJ_RESOURCES_UPDATED))
        transition = (not flags & OBJ_COND_EXISTS or bool(flags & OBJ_COND_TRUE) != (reason == AGGREGATE_SUCCESS)
                      or cond_reason != self.reason_ids[reason])
        required = propagated or transition
        write = bool(flags & OBJ_SCALARS_CHANGED) or required
        return ((OUT_CLUSTERS_CHANGED if differs else 0) | (OUT_CHANGES_PROPAGATED if propagated else 0)
                | (OUT_TRANSITION if transition else 0) | (OUT_UPDATE_REQUIRED if required else 0)
                | (OUT_STATUS_WRITE if write else 0))

    def apply(self, result: dict, now: str) -> List[FinishOutcome]:
        """The outputs of kad_sync_finish (or :func:`finish_numpy`) as objects. ``now``: the RFC 3339 time
        setPropagationCondition stamps (status.go:214), set exactly where it sets it."""
        a = self.finish_arrays()
        out = []
        for k, x in enumerate(self.objs):
            lo = int(a["ver_off"][k])
            hi = lo + int(result["ver_count"][k])
            cvs = [{"clusterName": self.names[int(c)], "version": self.versions[int(v)]}
                   for c, v in zip(result["out_ver_cluster"][lo:hi], result["out_ver_id"][lo:hi])]
            vstatus = {"templateVersion": x["template"], "overrideVersion": x["override"], "clusterVersions": cvs}
            if x["flags"] & OBJ_STATUS_ON_HOST:
                bits, reason, clusters = self._status_on_host(x)
            else:
                bits, reason = int(result["obj_out"][k]), self.reasons[int(result["reason_out"][k])]
                lo = int(a["st_off"][k])
                hi = lo + int(result["st_count"][k])
                clusters = [{"name": self.names[int(c)], "status": STATUS_NAMES[int(s)], **({"generation": int(g)} if g else {})}
                            for c, s, g in zip(result["out_st_cluster"][lo:hi], result["out_st_status"][lo:hi],
                                               result["out_st_gen"][lo:hi])]
            out.append(FinishOutcome(vstatus, bool(result["ver_write"][k]), self._new_status(x, bits, reason, clusters, now),
                                     bool(bits & OUT_STATUS_WRITE), reason, bool(bits & OUT_CLUSTERS_CHANGED)))
        return out

    @staticmethod
    def _new_status(x: dict, bits: int, reason: str, clusters: List[dict], now: str) -> dict:
        """The status update leaves (status.go:94-102, 139-153, 195-227), as its JSON: empty fields are omitted."""
        st = {k: v for k, v in x["status"].items() if k not in ("syncedGeneration", "collisionCount", "clusters", "conditions")}
        if x["generation"]:
            st["syncedGeneration"] = x["generation"]
        if x["collision"] is not None:
            st["collisionCount"] = x["collision"]
        if bits & OUT_CLUSTERS_CHANGED:
            if clusters:
                st["clusters"] = clusters
        elif x["status"].get("clusters"):
            st["clusters"] = x["status"]["clusters"]
        conds = [dict(c) if isinstance(c, dict) else c for c in x["status"].get("conditions") or []]
        cond = next((c for c in conds if isinstance(c, dict) and c.get("type") == PROPAGATION_CONDITION), None)
        if cond is None:
            cond = {"type": PROPAGATION_CONDITION}
            conds.append(cond)
        if bits & OUT_TRANSITION:
            cond["lastTransitionTime"] = now
            cond["status"] = "True" if reason == AGGREGATE_SUCCESS else "False"
            cond.pop("reason", None)
            if reason:
                cond["reason"] = reason
        if bits & OUT_UPDATE_REQUIRED:
            cond["lastUpdateTime"] = now
        st["conditions"] = conds
        return st


# ---------------------------------------------------------------------- the two calls, vectorised
def needs_update_numpy(n_clusters, row_obj, row_cluster, row_target, row_flags, obj_flags, rec_off, rec_cluster,
                       rec_version, ver_flags, **_) -> dict:
    """kad_sync_needs_update's outputs: the recorded versions looked up as sorted keys object * C + cluster."""
    C = max(int(n_clusters), 1)
    ro, rc, rt = (np.asarray(a, np.int64).reshape(-1) for a in (row_obj, row_cluster, row_target))
    rf, of, vf = (np.asarray(a, np.uint8).reshape(-1) for a in (row_flags, obj_flags, ver_flags))
    off = np.asarray(rec_off, np.int64).reshape(-1)
    keys = np.repeat(np.arange(len(off) - 1), np.diff(off)) * C + np.asarray(rec_cluster, np.int64).reshape(-1)
    ver = np.asarray(rec_version, np.int64).reshape(-1)
    want = ro * C + rc
    at = np.minimum(np.searchsorted(keys, want), max(len(keys) - 1, 0))
    hit = (keys[at] == want) & (of[ro] & 1).astype(bool) if len(keys) else np.zeros(len(want), bool)
    rec = np.where(hit, ver[at] if len(ver) else 0, 0)
    eq = ROW_REPLICAS_EQUAL | ROW_SURGE_EQUAL | ROW_UNAVAILABLE_EQUAL
    need = (rec != rt) | ((rf & eq) != eq) | (((vf[rt] & VER_IS_GEN) != 0) & ((rf & ROW_META_EQUIVALENT) == 0))
    return {"needs_update": need.astype(np.uint8), "recorded": rec.astype(np.int32)}


def _ranks(obj: np.ndarray, n_obj: int):
    """For ascending object indices: each element's rank within its object, and the counts per object."""
    count = np.bincount(obj, minlength=n_obj).astype(np.int64)
    first = np.concatenate(([0], np.cumsum(count)))[:-1]
    return np.arange(len(obj)) - first[obj], count


def finish_numpy(n_clusters, n_reasons, reason_check_clusters, reason_ns_not_federated, obj_flags, reason_in, cond_reason,
                 sel_off, sel_cluster, ent_off, ent_cluster, ent_status, ent_version, oldv_off, oldv_cluster, oldv_version,
                 olds_off, olds_cluster, olds_status, olds_gen, ver_gen, ver_flags, ver_off, st_off, **_) -> dict:
    """kad_sync_finish's outputs, vectorised over sorted keys object * C + cluster. Slots behind an object's counts
    hold 0."""
    C = max(int(n_clusters), 1)
    i64 = lambda a: np.asarray(a, np.int64).reshape(-1)  # noqa: E731
    of = np.asarray(obj_flags, np.uint16).reshape(-1).astype(np.int64)
    O_ = len(of)
    so, eo, vo, to, fo, go = (i64(a) for a in (sel_off, ent_off, oldv_off, olds_off, ver_off, st_off))
    obj_of = lambda off: np.repeat(np.arange(O_), np.diff(off))  # noqa: E731
    e_obj, v_obj, t_obj = obj_of(eo), obj_of(vo), obj_of(to)
    sk = obj_of(so) * C + i64(sel_cluster)
    ec, ev = i64(ent_cluster), i64(ent_version)
    ek = e_obj * C + ec
    es = _TRANSITION[np.asarray(ent_status, np.uint8).reshape(-1)]
    vf, vg = np.asarray(ver_flags, np.uint8).reshape(-1), i64(ver_gen)
    has_v, has_s = ev != 0, es != 0
    has_g = has_v & ((vf[ev] & VER_HAS_GEN) != 0)
    e_gen = np.where(has_g, vg[ev], 0)
    cur, on_host = (of & OBJ_VERSIONS_CURRENT) != 0, (of & OBJ_STATUS_ON_HOST) != 0
    # the new cluster versions (manager.go:170-181, 448-479)
    vc, vv = i64(oldv_cluster), i64(oldv_version)
    vk = v_obj * C + vc
    keep = cur[v_obj] & np.isin(vk, sk) & ~np.isin(vk, ek[has_v])
    nk = np.concatenate((ek[has_v], vk[keep]))
    nid = np.concatenate((ev[has_v], vv[keep]))
    order = np.argsort(nk, kind="stable")
    nk, nid = nk[order], nid[order]
    n_obj = nk // C
    rank, n_new = _ranks(n_obj, O_)
    cap_v = int(fo[-1]) if len(fo) else 0
    out_vc, out_vi = np.zeros(cap_v, np.int32), np.zeros(cap_v, np.int32)
    out_vc[fo[n_obj] + rank], out_vi[fo[n_obj] + rank] = nk % C, nid
    n_oldv = np.diff(vo)
    inside = rank < n_oldv[n_obj]
    at = np.minimum(vo[n_obj] + rank, max(len(vk) - 1, 0))
    mism = ~inside | ((vk[at] != nk) | (vv[at] != nid) if len(vk) else True)
    differ_v = (n_new != n_oldv) | (np.bincount(n_obj[mism], minlength=O_) > 0)
    ver_write = ((of & OBJ_VERSION_EXISTS) == 0) | ~cur | ((of & OBJ_OLDV_IRREGULAR) != 0) | \
        (((of & OBJ_OLDV_NIL) != 0) & (n_new == 0)) | differ_v
    # the status map, the generation map, clustersDiffers (status.go:159-179)
    s_obj = e_obj[has_s]
    s_rank, n_st = _ranks(s_obj, O_)
    n_gen = np.bincount(e_obj[has_g], minlength=O_)
    cap_s = int(go[-1]) if len(go) else 0
    out_sc, out_ss, out_sg = np.zeros(cap_s, np.int32), np.zeros(cap_s, np.uint8), np.zeros(cap_s, np.int64)
    live = ~on_host[s_obj]
    pos = (go[s_obj] + s_rank)[live]
    out_sc[pos], out_ss[pos], out_sg[pos] = ec[has_s][live], es[has_s][live], e_gen[has_s][live]
    n_olds = np.diff(to)
    tk = t_obj * C + i64(olds_cluster)
    at = np.minimum(np.searchsorted(ek, tk), max(len(ek) - 1, 0))
    hit = ek[at] == tk if len(ek) else np.zeros(len(tk), bool)
    s_now = np.where(hit, es[at] if len(es) else 0, 0)
    g_now = np.where(hit, e_gen[at] if len(es) else 0, 0)
    bad = (s_now != np.asarray(olds_status, np.uint8).reshape(-1)) | (g_now != i64(olds_gen))
    differs = (n_olds != n_st) | (n_olds != n_gen) | (np.bincount(t_obj[bad], minlength=O_) > 0)
    notok = np.bincount(e_obj[has_s & (es != ST_OK)], minlength=O_) > 0
    rin = i64(reason_in)
    reason = np.where((rin == 0) & notok, int(reason_check_clusters), rin)
    propagated = differs | ((n_st > 0) & ((of & OBJ_RESOURCES_UPDATED) != 0))
    transition = ((of & OBJ_COND_EXISTS) == 0) | (((of & OBJ_COND_TRUE) != 0) != (reason == 0)) | (i64(cond_reason) != reason)
    required = propagated | transition
    write = ((of & OBJ_SCALARS_CHANGED) != 0) | required
    bits = differs * OUT_CLUSTERS_CHANGED + propagated * OUT_CHANGES_PROPAGATED + transition * OUT_TRANSITION + \
        required * OUT_UPDATE_REQUIRED + write * OUT_STATUS_WRITE
    z = lambda a, dt: np.where(on_host, 0, a).astype(dt)  # noqa: E731
    return {"out_ver_cluster": out_vc, "out_ver_id": out_vi, "ver_count": n_new.astype(np.int32),
            "ver_write": ver_write.astype(np.uint8), "out_st_cluster": out_sc, "out_st_status": out_ss, "out_st_gen": out_sg,
            "st_count": z(n_st, np.int32), "obj_out": z(bits, np.uint8), "reason_out": z(reason, np.int32)}
