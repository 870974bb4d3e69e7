"""The federated-cluster controller's resource collection: node and pod resources per member cluster.

``updateClusterResources`` (pkg/controllers/federatedcluster/clusterstatus.go:162-202) runs every collection
interval for every ready member cluster: it lists the cluster's nodes and pods, counts the schedulable nodes
(``isNodeSchedulable``, util.go:114-132) and writes ``status.resources`` — Allocatable as the sum of the
schedulable nodes' allocatable lists, Available as Allocatable minus the requests of every pod that is not
Succeeded or Failed (``aggregateResources``, util.go:178-214; ``getPodResourceRequests``, :155-173). These are the
``allocatable`` / ``available`` columns the scheduler's snapshot is packed from.

This module holds the literal restatement over dicts with exact ``Fraction``s (:func:`is_node_schedulable`,
:func:`pod_resource_requests`, :func:`aggregate_resources`) and the batch form: :class:`ClusterStatusBatch` interns
resource names, picks one decimal scale per name, sorts every pod's entries and packs the clusters into the
arrays of ``kad_cluster_resources`` (include/kad_sched.h), which reduces them on the GPU; clusters outside the
device's number domain are computed by the host restatement instead. :meth:`ClusterStatusBatch.apply` writes the
results back.

Listing nodes and pods from member clusters is I/O and stays with the caller, as do the health check, API
discovery, conditions and joins.

Declared deviation: results are equal in value to the reference's (``Quantity.Equal``); the text written back is
the canonical decimal form of the value (``"2500m"``, ``"3221225472"``), where Go keeps the format of the first
non-zero operand (``"3Gi"``). The project reads quantities by value only.
"""

from __future__ import annotations

import dataclasses
from fractions import Fraction
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

from . import k8s
from . import types as T

NODE_SCHEDULABLE = 1                  # KAD_CS_NODE_SCHEDULABLE
POD_TERMINAL = 1                      # KAD_CS_POD_TERMINAL
KIND_CONTAINER, KIND_INIT, KIND_OVERHEAD = 0, 1, 2
MAX_RES = 64                          # resource names of one device call
VALUE_BOUND = 1 << 62                 # KAD_CS_VALUE_BOUND: max value x max entries of one cluster
SCALES = (0, 3, 6, 9)                 # a column holds value x 10^k
RESOURCE_PODS = "pods"                # corev1.ResourcePods
_SUFFIX = {0: "", 3: "m", 6: "u", 9: "n"}

Quantities = Dict[str, Fraction]


# ------------------------------------------------------------------ the reference, object by object
def _dict(v) -> dict:
    return v if isinstance(v, dict) else {}


def _list(v) -> list:
    return v if isinstance(v, list) else []


def is_node_schedulable(node: dict) -> bool:
    """isNodeSchedulable (util.go:114-132): false for spec.unschedulable, for a NoSchedule or NoExecute taint,
    and for a Ready condition whose status is not "True"; a PreferNoSchedule taint and a node without a Ready
    condition stay schedulable."""
    spec, status = _dict(node.get("spec")), _dict(node.get("status"))
    if spec.get("unschedulable"):
        return False
    for t in _list(spec.get("taints")):
        if _dict(t).get("effect") in (T.TAINT_NO_SCHEDULE, T.TAINT_NO_EXECUTE):
            return False
    for c in _list(status.get("conditions")):
        if _dict(c).get("type") == "Ready" and _dict(c).get("status") != "True":
            return False
    return True


def is_pod_terminal(pod: dict) -> bool:
    """util.go:200: a Succeeded or Failed pod holds no resources."""
    return _dict(pod.get("status")).get("phase") in ("Succeeded", "Failed")


def _resource_list(v) -> Quantities:
    return {n: k8s.quantity(q) for n, q in _dict(v).items()}


def _container_requests(c) -> Quantities:
    return _resource_list(_dict(_dict(c).get("resources")).get("requests"))


def pod_resource_requests(pod: dict) -> Quantities:
    """getPodResourceRequests (util.go:155-173): per name the sum over the containers, then for each init
    container in order the greater of it and the running value (an absent name is set), then the overhead."""
    spec = _dict(pod.get("spec"))
    reqs: Quantities = {}
    for c in _list(spec.get("containers")):
        for n, q in _container_requests(c).items():  # addResources
            reqs[n] = reqs[n] + q if n in reqs else q
    for c in _list(spec.get("initContainers")):
        for n, q in _container_requests(c).items():  # maxResources
            if n not in reqs or q > reqs[n]:
                reqs[n] = q
    if spec.get("overhead") is not None:
        for n, q in _resource_list(spec.get("overhead")).items():
            reqs[n] = reqs[n] + q if n in reqs else q
    return reqs


def aggregate_resources(nodes: Sequence[dict], pods: Sequence[dict]) -> Tuple[Quantities, Quantities]:
    """aggregateResources (util.go:178-214): (allocatable, available)."""
    allocatable: Quantities = {}
    for node in nodes:
        if not is_node_schedulable(node):
            continue
        for n, q in _resource_list(_dict(node.get("status")).get("allocatable")).items():
            allocatable[n] = allocatable[n] + q if n in allocatable else q
    allocatable.pop(RESOURCE_PODS, None)
    available = dict(allocatable)
    for pod in pods:
        if is_pod_terminal(pod):
            continue
        for n, q in pod_resource_requests(pod).items():
            if n in available:
                available[n] -= q
    return allocatable, available


def cluster_resources(nodes: Sequence[dict], pods: Sequence[dict]) -> Tuple[int, Quantities, Quantities]:
    """updateClusterResources (clusterstatus.go:187-199): (schedulableNodes, allocatable, available)."""
    alloc, avail = aggregate_resources(nodes, pods)
    return sum(1 for n in nodes if is_node_schedulable(n)), alloc, avail


# ------------------------------------------------------------------ number domain
def scale_of(q: Fraction) -> int:
    """The smallest k of SCALES at which q x 10^k is an integer (k8s.quantity yields nano precision)."""
    for k in SCALES:
        if (q * 10 ** k).denominator == 1:
            return k
    raise ValueError(f"quantity {q} finer than nano precision")


def format_quantity(q: Fraction) -> str:
    """The canonical decimal text of a value: an integer with the suffix of the smallest scale that holds it."""
    k = scale_of(q)
    return f"{int(q * 10 ** k)}{_SUFFIX[k]}"


def same_quantities(a: Optional[Dict[str, object]], b: Optional[Dict[str, object]]) -> bool:
    """Two ResourceLists equal name by name and value by value (Quantity.Equal)."""
    a, b = a or {}, b or {}
    return a.keys() == b.keys() and all(k8s.quantity(a[n]) == k8s.quantity(b[n]) for n in a)


# ------------------------------------------------------------------ the batch
HOST_NEGATIVE, HOST_NAMES, HOST_BOUND = "negative quantity", "more than 64 resource names", "value bound"


class ClusterStatusBatch:
    """The arrays of one kad_cluster_resources: per added cluster its nodes (schedulable flag, allocatable
    entries without ``pods``) and pods (terminal flag, request entries sorted by (resource, kind)), resource
    names interned in order of appearance, one scale per name. ``host``: {cluster index: reason} for the clusters
    the device's domain excludes; :meth:`results` computes those with :func:`cluster_resources`."""

    def __init__(self):
        self.names: List[str] = []
        self.at: Dict[str, int] = {}
        self.nodes: List[List[Tuple[int, List[Tuple[int, Fraction]]]]] = []
        self.pods: List[List[Tuple[int, List[Tuple[int, int, Fraction]]]]] = []
        self.raw: List[Tuple[Sequence[dict], Sequence[dict]]] = []
        self.host: Dict[int, str] = {}
        self.scales: List[int] = []
        self.device: List[int] = []  # the clusters of the device call, in its order

    def intern(self, name: str) -> int:
        i = self.at.get(name)
        if i is None:
            i = self.at[name] = len(self.names)
            self.names.append(name)
        return i

    def add(self, nodes: Sequence[dict], pods: Sequence[dict]) -> int:
        """One member cluster's listed nodes and pods; returns its index in the batch."""
        k = len(self.raw)
        self.raw.append((nodes, pods))
        nrec, prec = [], []
        for node in nodes:
            ents = [(self.intern(n), q) for n, q in _resource_list(_dict(node.get("status")).get("allocatable")).items()
                    if n != RESOURCE_PODS]
            nrec.append((NODE_SCHEDULABLE if is_node_schedulable(node) else 0, ents))
        for pod in pods:
            spec = _dict(pod.get("spec"))
            ents = []
            for kind, cs in ((KIND_CONTAINER, _list(spec.get("containers"))), (KIND_INIT, _list(spec.get("initContainers")))):
                for c in cs:
                    ents += [(self.intern(n), kind, q) for n, q in _container_requests(c).items()]
            if spec.get("overhead") is not None:
                ents += [(self.intern(n), KIND_OVERHEAD, q) for n, q in _resource_list(spec.get("overhead")).items()]
            ents.sort(key=lambda e: (e[0], e[1]))
            prec.append((POD_TERMINAL if is_pod_terminal(pod) else 0, ents))
        self.nodes.append(nrec)
        self.pods.append(prec)
        return k

    def _route_to_host(self) -> None:
        """Fill ``host``, ``scales`` and ``device``: negative quantities and names past the 64th first, then the
        scales over what is left, then the value bound (the cluster holding the largest value leaves until max
        value x max entries of one cluster fits, for node and for pod entries)."""
        self.host = {}
        K = len(self.raw)
        for k in range(K):
            qs = [e for _, ents in self.nodes[k] for e in ents] + [(e[0], e[2]) for _, ents in self.pods[k] for e in ents]
            if any(q < 0 for _, q in qs):
                self.host[k] = HOST_NEGATIVE
            elif any(r >= MAX_RES for r, _ in qs):
                self.host[k] = HOST_NAMES
        R = max(1, min(len(self.names), MAX_RES))
        self.scales = [0] * R
        for k in range(K):
            if k in self.host:
                continue
            for _, ents in self.nodes[k]:
                for r, q in ents:
                    self.scales[r] = max(self.scales[r], scale_of(q))
            for _, ents in self.pods[k]:
                for r, _, q in ents:
                    self.scales[r] = max(self.scales[r], scale_of(q))
        mul = [10 ** s for s in self.scales]
        for recs, val in ((self.nodes, lambda e: e[1] * mul[e[0]]), (self.pods, lambda e: e[2] * mul[e[0]])):
            live = [k for k in range(K) if k not in self.host]
            vmax = {k: max((val(e) for _, ents in recs[k] for e in ents), default=0) for k in live}
            cnt = {k: sum(len(ents) for _, ents in recs[k]) for k in live}
            by_val = sorted(live, key=lambda k: vmax[k], reverse=True)
            by_cnt = sorted(live, key=lambda k: cnt[k], reverse=True)
            gone, ci = set(), 0
            for k in by_val:
                while ci < len(by_cnt) and by_cnt[ci] in gone:
                    ci += 1
                emax = cnt[by_cnt[ci]] if ci < len(by_cnt) else 0
                if vmax[k] * emax <= VALUE_BOUND:
                    break
                gone.add(k)
                self.host[k] = HOST_BOUND
        self.device = [k for k in range(K) if k not in self.host]

    def arrays(self) -> dict:
        """The keyword arguments of runtime.cstat_args / Context.cluster_resources for the clusters of the
        device's domain (``device``)."""
        self._route_to_host()
        mul = [10 ** s for s in self.scales]
        cn, nf, ne, nr, nv = [0], [], [0], [], []
        cp, pf, pe, pr, pk, pv = [0], [], [0], [], [], []
        for k in self.device:
            for flags, ents in self.nodes[k]:
                nf.append(flags)
                for r, q in ents:
                    nr.append(r)
                    nv.append(int(q * mul[r]))
                ne.append(len(nr))
            cn.append(len(nf))
            for flags, ents in self.pods[k]:
                pf.append(flags)
                for r, kind, q in ents:
                    pr.append(r)
                    pk.append(kind)
                    pv.append(int(q * mul[r]))
                pe.append(len(pr))
            cp.append(len(pf))
        return dict(n_res=len(self.scales), cl_node_off=np.array(cn, np.int64), node_flags=np.array(nf, np.uint8),
                    node_ent_off=np.array(ne, np.int64), nent_res=np.array(nr, np.uint8), nent_val=np.array(nv, np.int64),
                    cl_pod_off=np.array(cp, np.int64), pod_flags=np.array(pf, np.uint8), pod_ent_off=np.array(pe, np.int64),
                    pent_res=np.array(pr, np.uint8), pent_kind=np.array(pk, np.uint8), pent_val=np.array(pv, np.int64))

    def results(self, r: Optional[dict]) -> List[Tuple[int, Quantities, Quantities]]:
        """Per added cluster (schedulableNodes, allocatable, available): the device clusters from
        kad_cluster_resources' outputs ``r`` (None when ``device`` is empty), the others from the host path."""
        out: List[Optional[Tuple[int, Quantities, Quantities]]] = [None] * len(self.raw)
        for k in self.host:
            out[k] = cluster_resources(*self.raw[k])
        R = len(self.scales)
        div = [10 ** s for s in self.scales]
        for j, k in enumerate(self.device):
            has = int(r["has"][j])
            alloc = {self.names[i]: Fraction(int(r["alloc"][j * R + i]), div[i]) for i in range(R) if has >> i & 1}
            avail = {self.names[i]: Fraction(int(r["avail"][j * R + i]), div[i]) for i in range(R) if has >> i & 1}
            out[k] = (int(r["sched_nodes"][j]), alloc, avail)
        return out  # type: ignore[return-value]

    def apply(self, r: Optional[dict], clusters: Sequence[T.FederatedCluster], objs: Optional[Sequence[dict]] = None
              ) -> Tuple[List[T.FederatedCluster], List[str]]:
        """Write the results back: ``objs[k]`` (FederatedCluster dicts, optional) get ``status.resources =
        {schedulableNodes, allocatable, available}`` in place; returns the cluster list with the new
        ``allocatable`` / ``available`` — a cluster whose quantities are equal in value is returned as it is, a
        changed one as a copy without resourceVersion (its content identifies it until the next read) — and the
        names of the changed clusters."""
        new, changed = [], []
        for k, (c, (sched, alloc, avail)) in enumerate(zip(clusters, self.results(r))):
            a = {n: format_quantity(q) for n, q in alloc.items()}
            v = {n: format_quantity(q) for n, q in avail.items()}
            if objs is not None:
                objs[k].setdefault("status", {})["resources"] = {"schedulableNodes": sched, "allocatable": dict(a),
                                                                 "available": dict(v)}
            if same_quantities(c.allocatable, a) and same_quantities(c.available, v):
                new.append(c)
            else:
                new.append(dataclasses.replace(c, allocatable=a, available=v, resource_version=""))
                changed.append(c.name)
        return new, changed


# ------------------------------------------------------------------ numpy restatement (cost comparison)
def cstat_numpy(n_res: int, **a) -> dict:
    """kad_cluster_resources restated with numpy on one thread over the same arrays: what the cost script
    compares the device with. Inputs are assumed valid."""
    R = int(n_res)
    cn, ne, cp, pe = a["cl_node_off"], a["node_ent_off"], a["cl_pod_off"], a["pod_ent_off"]
    K, N, P = len(cn) - 1, len(ne) - 1, len(pe) - 1
    node_cl = np.repeat(np.arange(K), np.diff(cn))
    sched = (a["node_flags"] & NODE_SCHEDULABLE) != 0
    ent_node = np.repeat(np.arange(N), np.diff(ne))
    m = sched[ent_node]
    key = node_cl[ent_node][m] * R + a["nent_res"][m].astype(np.int64)
    alloc = np.zeros(K * R, np.int64)
    np.add.at(alloc, key, a["nent_val"][m])
    present = np.zeros(K * R, bool)
    present[key] = True
    has = (present.reshape(K, R).astype(np.uint64) << np.arange(R, dtype=np.uint64)).sum(axis=1, dtype=np.uint64)
    sched_nodes = np.bincount(node_cl[sched], minlength=K).astype(np.int64)
    avail = alloc.copy()
    if len(a["pent_res"]):
        ent_pod = np.repeat(np.arange(P), np.diff(pe))
        run_key = ent_pod * R + a["pent_res"].astype(np.int64)  # non-decreasing: entries ascend by (res, kind)
        start = np.flatnonzero(np.r_[True, run_key[1:] != run_key[:-1]])
        val, kind = a["pent_val"], a["pent_kind"]
        csum = np.add.reduceat(np.where(kind == KIND_CONTAINER, val, 0), start)
        imax = np.maximum.reduceat(np.where(kind == KIND_INIT, val, 0), start)
        ovh = np.add.reduceat(np.where(kind == KIND_OVERHEAD, val, 0), start)
        req = np.maximum(csum, imax) + ovh
        pod_cl = np.repeat(np.arange(K), np.diff(cp))
        rp = ent_pod[start]
        k2 = pod_cl[rp] * R + a["pent_res"][start].astype(np.int64)
        live = ((a["pod_flags"][rp] & POD_TERMINAL) == 0) & present[k2]
        np.subtract.at(avail, k2[live], req[live])
    return {"alloc": alloc, "avail": avail, "has": has, "sched_nodes": sched_nodes}
