"""Follower scheduling: which objects follow which leaders, and where the followers go.

The follower controller (pkg/controllers/follower/controller.go) keeps, for every federated workload with
``enable-follower-scheduling: "true"``, the set of ConfigMaps, Secrets, PVCs and ServiceAccounts its pod
template references plus the objects its ``followers`` annotation names (``inferFollowers``, :354-378), and
sets each follower's ``spec.follows`` and its placement — the union of its leaders' placements
(``updateFollower`` / ``leaderPlacementUnion``, :380-421, 532-550) — under the controller name
``kubeadmiral.io/follower-controller``. This module restates the host side over object dicts:

* :func:`infer_followers` — ``getFollowersFromAnnotation`` + ``getFollowersFromPodTemplate``
  (follower/util.go:46-170) with the secret and configmap visitors of
  pkg/lifted/kubernetes/pkg/api/v1/pod/podutil.go:104-240;
* :class:`FollowerIndex` — the controller's two bidirectional caches (bidirectional_cache.go);
* :class:`FollowerPlacer` — the placement union and ``SetPlacementNames``' change test for a batch of
  followers in one ``kad_follower_union`` on the GPU, then the writes into the follower dicts.

Out of scope: informers, queues, the ``Update`` call, pending-controllers bookkeeping (:288-348).
"""

from __future__ import annotations

import json
from typing import Dict, Iterable, List, NamedTuple, Optional, Sequence, Set, Tuple

import numpy as np

from . import objects as O

CONTROLLER_NAME = "follower-controller"
PREFIXED_CONTROLLER_NAME = O.DEFAULT_PREFIX + CONTROLLER_NAME
FOLLOWERS_ANNOTATION = O.DEFAULT_PREFIX + "followers"  # common.FollowersAnnotation
FOLLOWS_PATH = ("spec", "follows")                     # common.FollowsPath

GroupKind = Tuple[str, str]

# controller.go:71-87
LEADER_POD_TEMPLATE_PATHS: Dict[GroupKind, str] = {
    ("apps", "Deployment"): "spec.template",
    ("apps", "StatefulSet"): "spec.template",
    ("apps", "DaemonSet"): "spec.template",
    ("batch", "Job"): "spec.template",
    ("batch", "CronJob"): "spec.jobTemplate.spec.template",
    ("", "Pod"): "spec",
}
SUPPORTED_FOLLOWER_TYPES = frozenset({
    ("", "ConfigMap"), ("", "Secret"), ("", "PersistentVolumeClaim"), ("", "ServiceAccount"), ("", "Service"),
    ("networking.k8s.io", "Ingress")})


class FollowerReference(NamedTuple):  # follower/util.go:34-38 (GroupKind = the federated type's)
    group: str
    kind: str
    namespace: str
    name: str


class LeaderReference(NamedTuple):  # types_follower.go:41-46
    group: str
    kind: str
    namespace: str
    name: str

    def to_json(self) -> dict:
        d = {}
        if self.group:
            d["group"] = self.group
        d["kind"] = self.kind
        if self.namespace:
            d["namespace"] = self.namespace
        d["name"] = self.name
        return d


class FollowerError(ValueError):
    """inferFollowers returns an error for this leader (the reconcile ends with StatusError)."""


def default_source_to_federated(group: str = "types.kubeadmiral.io") -> Dict[GroupKind, GroupKind]:
    """sourceToFederatedGKMap of a control plane that federates every supported follower type and every
    leader type as ``Federated<Kind>`` in ``group``."""
    return {gk: (group, "Federated" + gk[1]) for gk in list(SUPPORTED_FOLLOWER_TYPES) + list(LEADER_POD_TEMPLATE_PATHS)}


# ------------------------------------------------------------------ typed access to an unstructured pod spec
def _list(d: dict, key: str) -> list:
    v = d.get(key)
    if v is None:
        return []
    if not isinstance(v, list):
        raise FollowerError(f"{key}: expected a list, got {type(v).__name__}")
    return v


def _obj(d, key: str) -> Optional[dict]:
    v = d.get(key)
    if v is None:
        return None
    if not isinstance(v, dict):
        raise FollowerError(f"{key}: expected an object, got {type(v).__name__}")
    return v


def _str(d: dict, key: str) -> str:
    v = d.get(key)
    if v is None:
        return ""
    if not isinstance(v, str):
        raise FollowerError(f"{key}: expected a string, got {type(v).__name__}")
    return v


def _elems(d: dict, key: str) -> List[dict]:
    out = []
    for e in _list(d, key):
        if e is None:
            e = {}
        if not isinstance(e, dict):
            raise FollowerError(f"{key}: expected objects, got {type(e).__name__}")
        out.append(e)
    return out


def _containers(spec: dict) -> List[dict]:
    """VisitContainers with AllContainers (podutil.go:75-98): init, normal, ephemeral."""
    return _elems(spec, "initContainers") + _elems(spec, "containers") + _elems(spec, "ephemeralContainers")


def _ref_name(d: Optional[dict], key: str, field: str = "name") -> Optional[str]:
    """The name in d[key] when that reference is set (non-nil), else None."""
    r = _obj(d, key) if d is not None else None
    return None if r is None else _str(r, field)


# the volume sources VisitPodSecretNames switches over, in its case order (the first source set wins), with
# where each keeps its secret's name (podutil.go:118-167)
_SECRET_VOLUME_SOURCES = (
    ("azureFile", None, "secretName"), ("cephfs", "secretRef", "name"), ("cinder", "secretRef", "name"),
    ("flexVolume", "secretRef", "name"), ("projected", None, None), ("rbd", "secretRef", "name"),
    ("secret", None, "secretName"), ("scaleIO", "secretRef", "name"), ("iscsi", "secretRef", "name"),
    ("storageos", "secretRef", "name"), ("csi", "nodePublishSecretRef", "name"))


def pod_secret_names(spec: dict) -> Set[str]:
    """VisitPodSecretNames (podutil.go:104-188), empty names skipped."""
    names: List[Optional[str]] = [_str(r, "name") for r in _elems(spec, "imagePullSecrets")]
    for c in _containers(spec):
        names += [_ref_name(e, "secretRef") for e in _elems(c, "envFrom")]
        names += [_ref_name(_obj(e, "valueFrom"), "secretKeyRef") for e in _elems(c, "env")]
    for vol in _elems(spec, "volumes"):
        for key, ref, field in _SECRET_VOLUME_SOURCES:
            src = _obj(vol, key)
            if src is None:
                continue
            if key == "projected":
                names += [_ref_name(s, "secret") for s in _elems(src, "sources")]
            elif ref is None:
                names.append(_str(src, field))
            else:
                names.append(_ref_name(src, ref, field))
            break
    return {n for n in names if n}


def pod_configmap_names(spec: dict) -> Set[str]:
    """VisitPodConfigmapNames (podutil.go:194-236), empty names skipped."""
    names: List[Optional[str]] = []
    for c in _containers(spec):
        names += [_ref_name(e, "configMapRef") for e in _elems(c, "envFrom")]
        names += [_ref_name(_obj(e, "valueFrom"), "configMapKeyRef") for e in _elems(c, "env")]
    for vol in _elems(spec, "volumes"):
        proj = _obj(vol, "projected")
        if proj is not None:
            names += [_ref_name(s, "configMap") for s in _elems(proj, "sources")]
        elif _obj(vol, "configMap") is not None:
            names.append(_str(vol["configMap"], "name"))
    return {n for n in names if n}


def followers_from_pod(namespace: str, spec: dict, source_to_federated: Dict[GroupKind, GroupKind]
                       ) -> Set[FollowerReference]:
    """getFollowersFromPod (util.go:96-149) over a pod spec dict."""
    out: Set[FollowerReference] = set()
    gk = source_to_federated.get(("", "Secret"))
    if gk is not None:
        out |= {FollowerReference(*gk, namespace, n) for n in pod_secret_names(spec)}
    gk = source_to_federated.get(("", "ConfigMap"))
    if gk is not None:
        out |= {FollowerReference(*gk, namespace, n) for n in pod_configmap_names(spec)}
    gk = source_to_federated.get(("", "PersistentVolumeClaim"))
    if gk is not None:
        for vol in _elems(spec, "volumes"):
            pvc = _obj(vol, "persistentVolumeClaim")
            if pvc is not None:  # (an empty claim name is inserted as it is, util.go:128-134)
                out.add(FollowerReference(*gk, namespace, _str(pvc, "claimName")))
    gk = source_to_federated.get(("", "ServiceAccount"))
    if gk is not None:
        sa = _str(spec, "serviceAccountName")
        if sa:
            out.add(FollowerReference(*gk, namespace, sa))
    return out


def followers_from_annotation(obj: dict, source_to_federated: Dict[GroupKind, GroupKind]
                              ) -> Optional[Set[FollowerReference]]:
    """getFollowersFromAnnotation (util.go:46-78): followers come from the leader's namespace only."""
    text = (O.get_annotations(obj) or {}).get(FOLLOWERS_ANNOTATION, "")
    if not text:
        return None
    try:
        elems = json.loads(text)
    except ValueError as e:
        raise FollowerError(f"followers annotation: {e}") from None
    if elems is None:
        elems = []
    if not isinstance(elems, list):
        raise FollowerError("followers annotation: cannot unmarshal into []followerAnnotationElement")
    namespace = _meta_str(obj, "namespace")
    out: Set[FollowerReference] = set()
    for e in elems:
        if e is None:
            e = {}
        if not isinstance(e, dict):
            raise FollowerError("followers annotation: cannot unmarshal into followerAnnotationElement")
        source = (_str(e, "group"), _str(e, "kind"))
        gk = source_to_federated.get(source)
        if gk is None:
            raise FollowerError(f"no federated type config found for source type {_gk_string(source)}")
        out.add(FollowerReference(*gk, namespace, _str(e, "name")))
    return out


def _gk_string(gk: GroupKind) -> str:  # schema.GroupKind.String()
    return gk[1] if not gk[0] else f"{gk[1]}.{gk[0]}"


def _meta_str(obj: dict, field: str) -> str:
    meta = obj.get("metadata")
    v = meta.get(field) if isinstance(meta, dict) else None
    return v if isinstance(v, str) else ""


def pod_spec(obj: dict, pod_template_path: str) -> dict:
    """getPodSpec (util.go:151-170): the pod template under spec.template.<path> of a federated object."""
    v = obj
    for f in ("spec", "template") + tuple(pod_template_path.split(".")):
        if not isinstance(v, dict):
            raise FollowerError(f"pod template path {pod_template_path!r}: {f} is below a value that is not a map")
        if f not in v:
            raise FollowerError(f'pod template does not exist at path "{pod_template_path}"')
        v = v[f]
    if not isinstance(v, dict):
        raise FollowerError(f"pod template at path {pod_template_path!r} is not a map")
    return _obj(v, "spec") or {}


def source_group_kind(obj: dict) -> GroupKind:
    """The GroupKind of the object a federated object wraps (its spec.template)."""
    tmpl = obj.get("spec", {}).get("template", {}) if isinstance(obj.get("spec"), dict) else {}
    api = tmpl.get("apiVersion", "") if isinstance(tmpl, dict) else ""
    kind = tmpl.get("kind", "") if isinstance(tmpl, dict) else ""
    return (api.split("/")[0] if "/" in api else "", kind)


def infer_followers(obj: dict, source_gk: GroupKind, source_to_federated: Dict[GroupKind, GroupKind]
                    ) -> Optional[Set[FollowerReference]]:
    """inferFollowers (controller.go:354-378) for a leader of source type ``source_gk``: None when follower
    scheduling is not enabled on the object; raises :class:`FollowerError` where the reference returns one."""
    if (O.get_annotations(obj) or {}).get(O.ENABLE_FOLLOWER_SCHEDULING_ANNOTATION) != O.ANNOTATION_VALUE_TRUE:
        return None
    from_annotation = followers_from_annotation(obj, source_to_federated)
    spec = pod_spec(obj, LEADER_POD_TEMPLATE_PATHS.get(source_gk, ""))
    return (from_annotation or set()) | followers_from_pod(_meta_str(obj, "namespace"), spec, source_to_federated)


# ------------------------------------------------------------------ the controller's caches
class BidirectionalCache:
    """bidirectional_cache.go: key → values and value → keys, kept in step by update()."""

    def __init__(self):
        self.cache: Dict[object, set] = {}
        self.reverse: Dict[object, set] = {}

    def lookup(self, key) -> set:
        return set(self.cache.get(key, ()))

    def reverse_lookup(self, value) -> set:
        return set(self.reverse.get(value, ()))

    def update(self, key, new_values: Optional[Iterable]) -> None:
        new = set(new_values or ())
        old = self.cache.get(key, set())
        if new:
            self.cache[key] = new
        else:
            self.cache.pop(key, None)
        for v in old - new:
            keys = self.reverse.get(v)
            if keys is None:
                continue
            keys.discard(key)
            if not keys:
                del self.reverse[v]
        for v in new - old:
            self.reverse.setdefault(v, set()).add(key)


def current_leaders(follower_obj: dict) -> Set[LeaderReference]:
    """sets.New(followerObj.Spec.Follows...) (controller.go:470)."""
    spec = follower_obj.get("spec")
    follows = spec.get("follows") if isinstance(spec, dict) else None
    return {LeaderReference(f.get("group", ""), f.get("kind", ""), f.get("namespace", ""), f.get("name", ""))
            for f in (follows or []) if isinstance(f, dict)}


class FollowerIndex:
    """cacheObservedFromLeaders (leader → the followers it wants) and cacheObservedFromFollowers (follower →
    the leaders its spec.follows lists) of the controller (controller.go:311-312, 459-473)."""

    def __init__(self):
        self.from_leaders = BidirectionalCache()
        self.from_followers = BidirectionalCache()

    def update_leader(self, leader: LeaderReference, desired: Optional[Iterable[FollowerReference]]
                      ) -> Set[FollowerReference]:
        """reconcileLeader :311-324: record the leader's desired followers (None: the leader is gone or has
        follower scheduling off) and return the followers whose desired state may have changed."""
        self.from_leaders.update(leader, desired)
        return set(desired or ()) | self.from_followers.reverse_lookup(leader)

    def observe_follower(self, follower: FollowerReference, obj: Optional[dict]) -> Set[LeaderReference]:
        """reconcileFollower :457-471: record the leaders the follower object references (None: deleted)."""
        cur = current_leaders(obj) if obj is not None else set()
        self.from_followers.update(follower, cur)
        return cur

    def desired_leaders(self, follower: FollowerReference) -> Set[LeaderReference]:
        return self.from_leaders.reverse_lookup(follower)

    def leaders_changed(self, follower: FollowerReference, obj: dict) -> bool:
        """:475 — nil and empty sets are equal under equality.Semantic."""
        return self.desired_leaders(follower) != current_leaders(obj)

    def csr(self, followers: Sequence[FollowerReference], leader_index: Dict[LeaderReference, int]
            ) -> Tuple[np.ndarray, np.ndarray, List[List[LeaderReference]]]:
        """fol_off / fol_leader of kad_follower_union for ``followers``: each follower's desired leaders, sorted,
        as indices into the caller's leader list (-1: a leader absent from it). Also returns the sorted lists."""
        off = np.zeros(len(followers) + 1, np.int32)
        idx: List[int] = []
        lists = []
        for i, f in enumerate(followers):
            ls = sorted(self.desired_leaders(f))
            lists.append(ls)
            idx += [leader_index.get(ld, -1) for ld in ls]
            off[i + 1] = len(idx)
        return off, np.array(idx, np.int32), lists


def follower_reference(obj: dict) -> FollowerReference:
    """The reference of a federated follower object (its own group and kind)."""
    api = obj.get("apiVersion", "")
    return FollowerReference(api.split("/")[0] if "/" in api else "", obj.get("kind", ""), _meta_str(obj, "namespace"),
                             _meta_str(obj, "name"))


def leader_reference(obj: dict) -> LeaderReference:
    return LeaderReference(*follower_reference(obj))


def placement_names(obj: dict, controller: Optional[str] = None, exclude: Optional[str] = None) -> Optional[List[str]]:
    """The cluster names of ``controller``'s placement on the object (None: no such entry), or, with
    ``controller=None``, of every placement except ``exclude``'s (ClusterNameUnion over those)."""
    spec = obj.get("spec")
    pls = spec.get("placements") if isinstance(spec, dict) else None
    out: List[str] = []
    for p in pls or []:
        if not isinstance(p, dict):
            continue
        c = p.get("controller", "")
        if controller is not None and c != controller:
            continue
        if controller is None and exclude is not None and c == exclude:
            continue
        pl = p.get("placement") or {}
        out += [cl.get("name", "") for cl in (pl.get("clusters") or []) if isinstance(cl, dict)]
        if controller is not None:
            return out  # GetPlacementOrNil: the first entry of that controller
    return None if controller is not None else out


def set_follows(obj: dict, leaders: Sequence[LeaderReference]) -> None:
    """SetFollows (extensions_follower.go:27-38); the reference writes its set in map order, here sorted."""
    obj.setdefault("spec", {})["follows"] = [ld.to_json() for ld in sorted(leaders)]


class FollowerPlacer:
    """The placement half of updateFollower for a batch of followers: cluster names interned (the snapshot's
    ids first, other names after them), one kad_follower_union, then SetFollows and SetPlacementNames'
    writes into the follower dicts."""

    def __init__(self, ctx, snapshot):
        self.ctx = ctx
        self.C = snapshot.C
        self.names: List[str] = list(snapshot.names)
        self.at: Dict[str, int] = dict(snapshot.name_id)

    def intern(self, name: str) -> int:
        i = self.at.get(name)
        if i is None:
            i = self.at[name] = len(self.names)
            self.names.append(name)
        return i

    def csr(self, rows: Sequence[Optional[Iterable[str]]]) -> Tuple[np.ndarray, np.ndarray]:
        off = np.zeros(len(rows) + 1, np.int32)
        ids: List[int] = []
        for i, r in enumerate(rows):
            ids += [self.intern(n) for n in (r or ())]
            off[i + 1] = len(ids)
        return off, np.array(ids, np.int32)

    def union(self, fol_off, fol_leader, current: Sequence[Optional[Sequence[str]]], leaders=None, keep=None,
              sched=None, n_leaders: Optional[int] = None, emit_all: bool = False) -> dict:
        """One kad_follower_union. ``current[i]``: the names of follower i's follower-controller placement
        (None: no such placement); ``leaders`` / ``keep`` / ``sched``: per leader (per resident unit for
        ``sched``) the cluster names, or None (``leaders=None``: resident mode). Adds ``names``: per follower
        the union's names in id order (None where nothing was emitted for it)."""
        cur_off, cur_ids = self.csr(current)
        has = np.array([c is not None for c in current], np.uint8)
        args = {k: None if v is None else self.csr(v) for k, v in (("leaders", leaders), ("keep", keep), ("sched", sched))}
        r = self.ctx.follower_union(len(self.names), (fol_off, fol_leader, cur_off, cur_ids, has),
                                    n_leaders=n_leaders, emit_all=emit_all, **args)
        off, ids = r["out_off"], r["out_cluster"]
        r["names"] = [[self.names[j] for j in ids[off[i]:off[i + 1]]] if off[i + 1] > off[i] else None
                      for i in range(len(has))]
        return r

    def apply(self, followers: Sequence[dict], desired: Sequence[Sequence[LeaderReference]], fol_off, fol_leader,
              **leader_args) -> List[bool]:
        """updateFollower (controller.go:380-421) for every follower dict, in place: SetFollows where the desired
        leaders differ from spec.follows, the union under PREFIXED_CONTROLLER_NAME where the device reports
        SetPlacementNames' change — only those followers' names are sorted and written
        (objects.set_placement_cluster_names). Returns needsUpdate per follower."""
        current = [placement_names(f, PREFIXED_CONTROLLER_NAME) for f in followers]
        r = self.union(fol_off, fol_leader, current, **leader_args)
        out = []
        for i, f in enumerate(followers):
            leaders_changed = set(desired[i]) != current_leaders(f)
            if leaders_changed:
                set_follows(f, desired[i])
            if r["changed"][i]:
                O.set_placement_cluster_names(f, PREFIXED_CONTROLLER_NAME, set(r["names"][i] or ()))
            out.append(leaders_changed or bool(r["changed"][i]))
        return out
