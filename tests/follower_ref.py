"""Object-by-object checker for follower scheduling, written from the reference's Go with dicts and sets.

Independent of kubeadmiral_amd/follower.py: the tests run both and compare.

  infer_followers        controller.go:354-378 over follower/util.go:46-170 and the visitors of
                         pkg/lifted/kubernetes/pkg/api/v1/pod/podutil.go:104-240
  leader_placement_union controller.go:532-550
  set_placement_names    pkg/apis/types/v1alpha1/extensions_placements.go:78-103
  union_batch            the two above for a batch given as kad_follower_union's arrays
"""

import json

import numpy as np

ENABLE = "internal.kubeadmiral.io/enable-follower-scheduling"
FOLLOWERS = "kubeadmiral.io/followers"
POD_TEMPLATE_PATHS = {("apps", "Deployment"): "spec.template", ("apps", "StatefulSet"): "spec.template",
                      ("apps", "DaemonSet"): "spec.template", ("batch", "Job"): "spec.template",
                      ("batch", "CronJob"): "spec.jobTemplate.spec.template", ("", "Pod"): "spec"}


class RefError(Exception):
    pass


def _get(d, *path):
    """d[path...] or None as soon as something on the way is missing or null."""
    for p in path:
        if not isinstance(d, dict) or d.get(p) is None:
            return None
        d = d[p]
    return d


def visit_containers(spec):
    for kind in ("initContainers", "containers", "ephemeralContainers"):
        for c in spec.get(kind) or []:
            yield c or {}


def visit_secret_names(spec, visit):
    for ref in spec.get("imagePullSecrets") or []:
        visit(_get(ref, "name"))
    for c in visit_containers(spec):
        for env in c.get("envFrom") or []:
            if _get(env, "secretRef") is not None:
                visit(_get(env, "secretRef", "name"))
        for var in c.get("env") or []:
            if _get(var, "valueFrom", "secretKeyRef") is not None:
                visit(_get(var, "valueFrom", "secretKeyRef", "name"))
    for vol in spec.get("volumes") or []:
        # a Go switch: the first case that holds is the only one taken
        if _get(vol, "azureFile") is not None:
            visit(_get(vol, "azureFile", "secretName"))
        elif _get(vol, "cephfs") is not None:
            if _get(vol, "cephfs", "secretRef") is not None:
                visit(_get(vol, "cephfs", "secretRef", "name"))
        elif _get(vol, "cinder") is not None:
            if _get(vol, "cinder", "secretRef") is not None:
                visit(_get(vol, "cinder", "secretRef", "name"))
        elif _get(vol, "flexVolume") is not None:
            if _get(vol, "flexVolume", "secretRef") is not None:
                visit(_get(vol, "flexVolume", "secretRef", "name"))
        elif _get(vol, "projected") is not None:
            for src in _get(vol, "projected", "sources") or []:
                if _get(src, "secret") is not None:
                    visit(_get(src, "secret", "name"))
        elif _get(vol, "rbd") is not None:
            if _get(vol, "rbd", "secretRef") is not None:
                visit(_get(vol, "rbd", "secretRef", "name"))
        elif _get(vol, "secret") is not None:
            visit(_get(vol, "secret", "secretName"))
        elif _get(vol, "scaleIO") is not None:
            if _get(vol, "scaleIO", "secretRef") is not None:
                visit(_get(vol, "scaleIO", "secretRef", "name"))
        elif _get(vol, "iscsi") is not None:
            if _get(vol, "iscsi", "secretRef") is not None:
                visit(_get(vol, "iscsi", "secretRef", "name"))
        elif _get(vol, "storageos") is not None:
            if _get(vol, "storageos", "secretRef") is not None:
                visit(_get(vol, "storageos", "secretRef", "name"))
        elif _get(vol, "csi") is not None:
            if _get(vol, "csi", "nodePublishSecretRef") is not None:
                visit(_get(vol, "csi", "nodePublishSecretRef", "name"))


def visit_configmap_names(spec, visit):
    for c in visit_containers(spec):
        for env in c.get("envFrom") or []:
            if _get(env, "configMapRef") is not None:
                visit(_get(env, "configMapRef", "name"))
        for var in c.get("env") or []:
            if _get(var, "valueFrom", "configMapKeyRef") is not None:
                visit(_get(var, "valueFrom", "configMapKeyRef", "name"))
    for vol in spec.get("volumes") or []:
        if _get(vol, "projected") is not None:
            for src in _get(vol, "projected", "sources") or []:
                if _get(src, "configMap") is not None:
                    visit(_get(src, "configMap", "name"))
        elif _get(vol, "configMap") is not None:
            visit(_get(vol, "configMap", "name"))


def _collect(visitor, spec):
    got = set()
    visitor(spec, lambda n: got.add(n) if n else None)  # skipEmptyNames
    return got


def secret_names(spec):
    return _collect(visit_secret_names, spec)


def configmap_names(spec):
    return _collect(visit_configmap_names, spec)


def followers_from_pod(namespace, spec, s2f):
    """getFollowersFromPod: a set of (federated group, federated kind, namespace, name)."""
    out = set()
    if ("", "Secret") in s2f:
        out |= {s2f[("", "Secret")] + (namespace, n) for n in secret_names(spec)}
    if ("", "ConfigMap") in s2f:
        out |= {s2f[("", "ConfigMap")] + (namespace, n) for n in configmap_names(spec)}
    if ("", "PersistentVolumeClaim") in s2f:
        for vol in spec.get("volumes") or []:
            if _get(vol, "persistentVolumeClaim") is not None:
                out.add(s2f[("", "PersistentVolumeClaim")] + (namespace, _get(vol, "persistentVolumeClaim", "claimName") or ""))
    if ("", "ServiceAccount") in s2f and spec.get("serviceAccountName"):
        out.add(s2f[("", "ServiceAccount")] + (namespace, spec["serviceAccountName"]))
    return out


def infer_followers(obj, source_gk, s2f):
    ann = _get(obj, "metadata", "annotations") or {}
    if ann.get(ENABLE) != "true":
        return None
    ns = _get(obj, "metadata", "namespace") or ""
    out = set()
    if ann.get(FOLLOWERS):
        try:
            elems = json.loads(ann[FOLLOWERS])
        except ValueError as e:
            raise RefError(str(e))
        if elems is not None and not isinstance(elems, list):
            raise RefError("json: cannot unmarshal into Go value of type []follower.followerAnnotationElement")
        for e in elems or []:
            e = e or {}
            gk = (e.get("group", ""), e.get("kind", ""))
            if gk not in s2f:
                raise RefError("no federated type config found for source type %s" % (gk,))
            out.add(s2f[gk] + (ns, e.get("name", "")))
    path = POD_TEMPLATE_PATHS.get(source_gk, "")
    tmpl = obj
    for f in ["spec", "template"] + path.split("."):
        if not isinstance(tmpl, dict) or f not in tmpl:
            raise RefError('pod template does not exist at path "%s"' % path)
        tmpl = tmpl[f]
    if not isinstance(tmpl, dict):
        raise RefError("pod template is not a map")
    return out | followers_from_pod(ns, tmpl.get("spec") or {}, s2f)


def leader_placement_union(leaders, leader_sets):
    """leaders: indices into leader_sets or -1 / an index whose set is None (absent from the store)."""
    clusters = set()
    for ld in leaders:
        if ld < 0 or leader_sets[ld] is None:
            continue
        clusters |= set(leader_sets[ld])
    return clusters


def set_placement_names(current, new):
    """current: the controller's placement clusters as a list, or None when it has no entry. Returns
    (hasChange, the clusters afterwards or None when the entry is gone)."""
    if len(new) == 0:
        return current is not None, None
    if set(new) != set(current or []):
        return True, sorted(new)
    return False, current


def union_batch(followers, leader_sets, emit_all=False):
    """followers = (fol_off, fol_leader, cur_off, cur_cluster, cur_has); leader_sets: per leader a set of ids.
    Returns changed, count, out_off, out_cluster as kad_follower_union defines them."""
    fo, fl, co, cc, ch = followers
    F = len(ch)
    changed = np.zeros(F, np.uint8)
    count = np.zeros(F, np.int32)
    off = np.zeros(F + 1, np.int64)
    out = []
    for i in range(F):
        u = leader_placement_union([int(x) for x in fl[fo[i]:fo[i + 1]]], leader_sets)
        # (a placement entry that does not exist holds no clusters: cur_has = 0 comes with an empty range)
        cur = [int(x) for x in cc[co[i]:co[i + 1]]] if ch[i] else None
        changed[i] = set_placement_names(cur, u)[0]
        count[i] = len(u)
        if changed[i] or emit_all:
            out += sorted(u)
        off[i + 1] = len(out)
    return changed, count, off, np.array(out, np.int32)


def resident_leader_sets(status, count, cluster, out_off, cur_off, cur_id, n_leaders, sched=None, keep=None):
    """The leaders' id sets of resident mode, from the downloaded results of the schedule (status, count,
    cluster by out_off), the batch's CurrentClusters ids and the caller's sched / keep CSRs."""
    W = len(status)
    sets = []
    for i in range(n_leaders):
        s = set()
        if i < W:
            st = int(status[i])
            if st == 0:
                s |= {int(x) for x in cluster[out_off[i]:out_off[i] + count[i]]}
            elif st == 1:
                s |= {int(x) for x in cur_id[cur_off[i]:cur_off[i + 1]] if x >= 0}
            elif st != 2 and sched is not None:
                s |= {int(x) for x in sched[1][sched[0][i]:sched[0][i + 1]]}
        if keep is not None:
            s |= {int(x) for x in keep[1][keep[0][i]:keep[0][i + 1]]}
        sets.append(s)
    return sets
