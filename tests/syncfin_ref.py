"""The second half of syncToClusters for one object, restated from the Go line by line: dicts keyed by cluster name
and real version strings, no interning, no arrays. Shares nothing with kubeadmiral_amd.syncfin's packing.

  needs_update   util.ObjectNeedsUpdate (pkg/controllers/util/propagatedversion.go:54-119)
  version_get    VersionManager.Get (pkg/controllers/sync/version/manager.go:119-148)
  finish         dispatcher.Wait's transitions (sync/dispatch/managed.go:137-155), VersionManager.Update
                 (manager.go:152-210, 448-479), CollectedStatus (managed.go:642-654), setFederatedStatus
                 (sync/controller.go:637-656) and status.update (sync/status/status.go:87-229)
"""
import copy

NOW = "2024-05-06T07:08:09Z"


class _Err(Exception):
    pass


def _nested(obj, fields):  # unstructured.NestedFieldNoCopy
    val = obj
    for f in fields:
        if not isinstance(val, dict):
            raise _Err()
        if f not in val:
            return None, False
        val = val[f]
    return val, True


def _nested_int64(obj, fields):
    val, found = _nested(obj, fields)
    if not found:
        return 0, False
    if not isinstance(val, int) or isinstance(val, bool):
        raise _Err()
    return val, True


def _nested_string(obj, fields):
    val, found = _nested(obj, fields)
    if not found:
        return "", False
    if not isinstance(val, str):
        raise _Err()
    return val, True


def _get_int64_from_path(obj, path):  # utilunstructured.GetInt64FromPath: (*int64, error)
    v, exists = _nested_int64(obj, [p for p in path.split(".") if p])
    return v if exists else None


def object_version(obj):  # propagatedversion.go:43-49
    md = obj.get("metadata", {})
    generation = md.get("generation", 0)
    if generation != 0:
        return "gen:%d" % generation
    return "rv:" + md.get("resourceVersion", "")


def _string_map(obj, key):
    m = obj.get("metadata", {}).get(key)
    if not isinstance(m, dict) or any(not isinstance(v, str) for v in m.values()):
        return None
    return m


def _meta_equivalent(a, b):  # util/meta.go:90-108
    if a.get("metadata", {}).get("name", "") != b.get("metadata", {}).get("name", ""):
        return False
    if a.get("metadata", {}).get("namespace", "") != b.get("metadata", {}).get("namespace", ""):
        return False
    for key in ("labels", "annotations"):
        x, y = _string_map(a, key), _string_map(b, key)
        deep_equal = (x is None) == (y is None) and (x or {}) == (y or {})
        if not deep_equal and (len(x or {}) != 0 or len(y or {}) != 0):
            return False
    return True


def _int_or_string_current(desired, cluster_obj, fields):  # propagatedversion.go:78-92
    need_update = True
    try:
        d, ok = _nested_string(desired, fields)
    except _Err:
        try:
            d, ok = _nested_int64(desired, fields)
        except _Err:
            return need_update
        try:
            c, ok2 = _nested_int64(cluster_obj, fields)
        except _Err:
            return need_update
        if ok == ok2 and d == c:
            need_update = False
        return need_update
    try:
        c, ok2 = _nested_string(cluster_obj, fields)
    except _Err:
        return need_update
    if ok == ok2 and d == c:
        need_update = False
    return need_update


def needs_update(desired, cluster_obj, recorded_version, replicas_spec):
    target_version = object_version(cluster_obj)
    if recorded_version != target_version:
        return True
    need_update = True
    try:
        d = _get_int64_from_path(desired, replicas_spec)
        try:
            c = _get_int64_from_path(cluster_obj, replicas_spec)
            if (d is None and c is None) or (d is not None and c is not None and d == c):
                need_update = False
        except _Err:
            pass
    except _Err:
        pass
    if need_update:
        return True
    if _int_or_string_current(desired, cluster_obj, ["spec", "strategy", "rollingUpdate", "maxSurge"]):
        return True
    if _int_or_string_current(desired, cluster_obj, ["spec", "strategy", "rollingUpdate", "maxUnavailable"]):
        return True
    return target_version.startswith("gen:") and not _meta_equivalent(desired, cluster_obj)


def version_get(stored, template_version, override_version):
    version_map = {}
    if stored is None:
        return version_map
    if template_version == stored.get("templateVersion", "") and override_version == stored.get("overrideVersion", ""):
        for cv in stored.get("clusterVersions") or []:
            version_map[cv.get("clusterName", "")] = cv.get("version", "")
    return version_map


def _parse_int64(s):  # strconv.ParseInt(s, 10, 64) → (value, ok)
    digits = s[1:] if s[:1] in ("+", "-") else s
    if digits == "" or any(ch not in "0123456789" for ch in digits):
        return 0, False
    n = int(digits)
    if s[:1] == "-":
        n = -n
    if n < -(1 << 63) or n > (1 << 63) - 1:
        return 0, False
    return n, True


def generation_map(version_map):  # propagatedversion.go:138-157
    out = {}
    for key, version in version_map.items():
        if version.startswith("rv:"):
            out[key] = 0
            continue
        if not version.startswith("gen:"):
            continue
        g, ok = _parse_int64(version[len("gen:"):])
        if not ok:
            continue
        out[key] = g
    return out


def _cluster_versions(version_map):  # VersionMapToClusterVersions (manager.go:465-479)
    out = [{"clusterName": n, "version": v} for n, v in version_map.items() if v != ""]
    out.sort(key=lambda cv: cv["clusterName"].encode())
    return out


def finish(obj, now=NOW):
    """obj: status (the stored status or None), generation, collision, selected, records {cluster: (status as the
    operations left it, version recorded or "")}, resources_updated, stored_version (or None), template, override,
    reason, nnf → what the reference leaves behind."""
    # ---- Wait (managed.go:137-155)
    status_map = {n: s for n, (s, _) in obj["records"].items() if s != ""}
    for key, value in list(status_map.items()):
        if value in ("CreationTimedOut", "UpdateTimedOut"):
            status_map[key] = "OK"
        elif value == "DeletionTimedOut":
            status_map[key] = "WaitingForRemoval"
        elif value == "LabelRemovalTimedOut":
            del status_map[key]
    version_map = {n: v for n, (_, v) in obj["records"].items() if v != ""}
    # ---- VersionManager.Update (manager.go:152-210)
    stored = obj["stored_version"]
    new_versions = dict(version_map)
    if stored is not None:
        cluster_versions = None
        if stored.get("templateVersion", "") == obj["template"] and stored.get("overrideVersion", "") == obj["override"]:
            cluster_versions = stored.get("clusterVersions")
        selected = set(obj["selected"])
        for old in cluster_versions or []:  # updateClusterVersions (manager.go:448-463)
            if old.get("clusterName", "") not in selected:
                continue
            if old.get("clusterName", "") not in new_versions:
                new_versions[old.get("clusterName", "")] = old.get("version", "")
    new_list = _cluster_versions(new_versions)
    version_status = {"templateVersion": obj["template"], "overrideVersion": obj["override"], "clusterVersions": new_list}
    version_write = True
    if stored is not None:
        old_list = stored.get("clusterVersions")
        deep_equal = old_list is not None and [(c.get("clusterName", ""), c.get("version", "")) for c in old_list] == \
            [(c["clusterName"], c["version"]) for c in new_list]
        if stored.get("templateVersion", "") == obj["template"] and stored.get("overrideVersion", "") == obj["override"] \
                and deep_equal:
            version_write = False
    # ---- CollectedStatus, setFederatedStatus, update
    gen_map = generation_map(version_map)
    reason = obj["reason"]
    if reason == "" and obj["nnf"]:
        reason = "NamespaceNotFederated"
    s = copy.deepcopy(obj["status"]) if obj["status"] is not None else {}
    generation_updated = s.get("syncedGeneration", 0) != obj["generation"]
    if generation_updated:
        s["syncedGeneration"] = obj["generation"]
    collision_updated = s.get("collisionCount") != obj["collision"]
    if collision_updated:
        s["collisionCount"] = obj["collision"]
    if reason == "":
        for value in status_map.values():
            if value != "OK":
                reason = "CheckClusters"
                break
    # setClusters / clustersDiffers
    old_clusters = s.get("clusters") or []
    differs = len(old_clusters) != len(status_map) or len(old_clusters) != len(gen_map)
    if not differs:
        for st in old_clusters:
            if status_map.get(st.get("name", ""), "") != st.get("status", ""):
                differs = True
                break
            if gen_map.get(st.get("name", ""), 0) != st.get("generation", 0):
                differs = True
                break
    if differs:
        s["clusters"] = [{"name": n, "status": status_map[n], "generation": gen_map.get(n, 0)}
                         for n in sorted(status_map, key=lambda n: n.encode())]
    changes_propagated = differs or (len(status_map) > 0 and obj["resources_updated"])
    # setPropagationCondition
    new_status = "True" if reason == "" else "False"
    conds = s.get("conditions") or []
    s["conditions"] = conds
    cond = None
    for c in conds:
        if c.get("type") == "Propagation":
            cond = c
            break
    new_condition = cond is None
    if new_condition:
        cond = {"type": "Propagation"}
        conds.append(cond)
    transition = new_condition or not (cond.get("status", "") == new_status and cond.get("reason", "") == reason)
    if transition:
        cond["lastTransitionTime"] = now
        cond["status"] = new_status
        cond["reason"] = reason
    update_required = changes_propagated or transition
    if update_required:
        cond["lastUpdateTime"] = now
    status_write = generation_updated or collision_updated or update_required
    return {"version_status": version_status, "version_write": version_write, "status": _omitempty(s),
            "status_write": status_write, "reason": reason, "clusters_changed": differs}


def _omitempty(s):
    """The status as its JSON (types_status.go:38-66): zero numbers, empty strings and empty slices are omitted."""
    out = {k: v for k, v in s.items() if k not in ("syncedGeneration", "collisionCount", "clusters", "conditions")}
    if s.get("syncedGeneration", 0):
        out["syncedGeneration"] = s["syncedGeneration"]
    if s.get("collisionCount") is not None:
        out["collisionCount"] = s["collisionCount"]
    if s.get("clusters"):
        out["clusters"] = [{k: v for k, v in c.items() if k == "name" or v not in ("", 0)} for c in s["clusters"]]
    if s.get("conditions"):
        out["conditions"] = [{k: v for k, v in c.items() if k in ("type", "status") or v != ""} for c in s["conditions"]]
    return out
