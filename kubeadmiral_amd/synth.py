"""Deterministic synthetic workloads (BASELINE.json configs).

There is no cluster or dataset here, so every benchmark and parity run uses
seeded synthetic FederatedCluster snapshots and SchedulingUnit batches with the
shapes and distributions of SURVEY.md §8(d):

* ``c1`` 1k Deployment units × 16 clusters, default plugins, Divide (seed 0xC1)
* ``c2`` 100k × 256: Fit + Taint + Affinity filters, LeastAllocated, MaxCluster, Duplicate (0xC2)
* ``c3`` 1M × 1k, same generator as c2 (0xC3)
* ``c4`` 1M Divide units × 512 clusters: weights, min/max, capacity caps (0xC4)
* ``c5`` 100k × 10k adversarial filters (0xC5)
* ``fuzz`` small batches exercising every branch and edge case of the path

``scale`` shrinks W (and C for c5) so tests can run the same generators on CPU.
"""

from __future__ import annotations

from typing import Dict, List, Optional, Tuple

import json

import numpy as np

from . import framework as F
from . import k8s
from . import types as T

GI = 1 << 30
TI = 1 << 40
EFFECTS = [T.TAINT_NO_SCHEDULE, T.TAINT_PREFER_NO_SCHEDULE, T.TAINT_NO_EXECUTE]
GVKS = [("apps", "v1", "Deployment"), ("apps", "v1", "StatefulSet"), ("apps", "v1", "DaemonSet"),
        ("batch", "v1", "Job"), ("", "v1", "ConfigMap"), ("", "v1", "Service"), ("batch", "v1", "CronJob"),
        ("networking.k8s.io", "v1", "Ingress")]

SEEDS = {"c1": 0xC1, "c2": 0xC2, "c3": 0xC3, "c4": 0xC4, "c5": 0xC5, "c3r": 0xC3, "c3p": 0xC3}
SIZES = {"c1": (1000, 16), "c2": (100_000, 256), "c3": (1_000_000, 1000), "c4": (1_000_000, 512),
         "c5": (100_000, 10_000), "c3r": (1_000_000, 1000), "c3p": (1_000_000, 1000)}


def production_resources(clusters, rng: np.random.Generator, p_over: float = 0.015, p_empty: float = 0.005):
    """``clusters`` (in place) with the resource shapes aggregateResources
    (pkg/controllers/federatedcluster/util.go:178-214) reports for real member clusters: nodes that are
    Unschedulable, NotReady or carry a NoSchedule / NoExecute taint (isNodeSchedulable, :114-131) are left out
    of allocatable, while every non-terminal pod's requests are still subtracted from available (:199-210) —
    * a fraction ``p_over`` of clusters whose pods on left-out nodes push cpu and / or memory available
      below 0 (used = allocatable - available above allocatable by up to 30 %);
    * a fraction ``p_empty`` whose every node is left out: empty Allocatable and Available lists
      (allocatable 0, used 0 — pods subtract only from resources present, :203-207).
    Returns the indices of the two groups."""
    C = len(clusters)
    u = rng.random(C)
    over = np.nonzero(u < p_over)[0]
    empty = np.nonzero((u >= p_over) & (u < p_over + p_empty))[0]
    for c in over:
        cl = clusters[int(c)]
        which = int(rng.integers(1, 4))  # 1 cpu, 2 memory, 3 both
        if which & 1 and "cpu" in (cl.allocatable or {}):
            ac = k8s.milli_value(k8s.quantity(cl.allocatable["cpu"]))
            cl.available = dict(cl.available or {}, cpu=f"{-int(ac * rng.uniform(0.001, 0.3))}m")
        if which & 2 and "memory" in (cl.allocatable or {}):
            am = k8s.value(k8s.quantity(cl.allocatable["memory"]))
            cl.available = dict(cl.available or {}, memory=str(-int(am * rng.uniform(0.001, 0.3))))
    for c in empty:
        clusters[int(c)].allocatable = {}
        clusters[int(c)].available = {}
    return over, empty

# ------------------------------------------------------- production-shaped API-resource lists
# What a member cluster's discovery returns (kube 1.26 built-ins and commonly installed operators' CRDs), as
# FederatedCluster.Status.APIResourceTypes holds it: updateClusterAPIResources
# (pkg/controllers/federatedcluster/clusterstatus.go:204-268) keeps every resource of every group version
# whose name has no "/" (subresources skipped, :239-241) and sorts the list by Kind (:262-264). The same Kind
# appears under several group versions (autoscaling/v1 and v2 HorizontalPodAutoscaler, core and events.k8s.io
# Event, ...). Go's sort.Slice is unstable, so the order among equal Kinds is pdqsort's; here it is discovery
# order (a stable sort) — the order only decides the snapshot's GVK ids, never a scheduling result.
_BUILTIN_API = [
    ("", "v1", ["Binding", "ComponentStatus", "ConfigMap", "Endpoints", "Event", "LimitRange", "Namespace", "Node",
                "PersistentVolumeClaim", "PersistentVolume", "Pod", "PodTemplate", "ReplicationController",
                "ResourceQuota", "Secret", "ServiceAccount", "Service"]),
    ("admissionregistration.k8s.io", "v1", ["MutatingWebhookConfiguration", "ValidatingWebhookConfiguration"]),
    ("apiextensions.k8s.io", "v1", ["CustomResourceDefinition"]),
    ("apiregistration.k8s.io", "v1", ["APIService"]),
    ("apps", "v1", ["ControllerRevision", "DaemonSet", "Deployment", "ReplicaSet", "StatefulSet"]),
    ("authentication.k8s.io", "v1", ["TokenReview"]),
    ("authorization.k8s.io", "v1", ["LocalSubjectAccessReview", "SelfSubjectAccessReview", "SelfSubjectRulesReview",
                                    "SubjectAccessReview"]),
    ("autoscaling", "v1", ["HorizontalPodAutoscaler"]),
    ("autoscaling", "v2", ["HorizontalPodAutoscaler"]),
    ("batch", "v1", ["CronJob", "Job"]),
    ("certificates.k8s.io", "v1", ["CertificateSigningRequest"]),
    ("coordination.k8s.io", "v1", ["Lease"]),
    ("discovery.k8s.io", "v1", ["EndpointSlice"]),
    ("events.k8s.io", "v1", ["Event"]),
    ("flowcontrol.apiserver.k8s.io", "v1beta2", ["FlowSchema", "PriorityLevelConfiguration"]),
    ("flowcontrol.apiserver.k8s.io", "v1beta3", ["FlowSchema", "PriorityLevelConfiguration"]),
    ("networking.k8s.io", "v1", ["IngressClass", "Ingress", "NetworkPolicy"]),
    ("node.k8s.io", "v1", ["RuntimeClass"]),
    ("policy", "v1", ["PodDisruptionBudget"]),
    ("rbac.authorization.k8s.io", "v1", ["ClusterRoleBinding", "ClusterRole", "RoleBinding", "Role"]),
    ("scheduling.k8s.io", "v1", ["PriorityClass"]),
    ("storage.k8s.io", "v1", ["CSIDriver", "CSINode", "CSIStorageCapacity", "StorageClass", "VolumeAttachment"]),
    ("metrics.k8s.io", "v1beta1", ["NodeMetrics", "PodMetrics"]),
]
# operators: a cluster has each one's whole group (p = 0.9), so some clusters lack a kind (API-resource gaps)
_OPERATOR_API = [
    ("cert-manager.io", "v1", ["Certificate", "CertificateRequest", "ClusterIssuer", "Issuer"]),
    ("acme.cert-manager.io", "v1", ["Challenge", "Order"]),
    ("monitoring.coreos.com", "v1", ["Alertmanager", "PodMonitor", "Probe", "Prometheus", "PrometheusRule",
                                     "ServiceMonitor", "ThanosRuler"]),
    ("monitoring.coreos.com", "v1alpha1", ["AlertmanagerConfig"]),
    ("argoproj.io", "v1alpha1", ["AnalysisRun", "AnalysisTemplate", "ClusterAnalysisTemplate", "Experiment",
                                 "Rollout"]),
    ("apps.kruise.io", "v1alpha1", ["AdvancedCronJob", "BroadcastJob", "CloneSet", "DaemonSet", "ImagePullJob",
                                    "NodeImage", "ResourceDistribution", "SidecarSet", "UnitedDeployment",
                                    "WorkloadSpread"]),
    ("apps.kruise.io", "v1beta1", ["StatefulSet"]),
    ("snapshot.storage.k8s.io", "v1", ["VolumeSnapshotClass", "VolumeSnapshotContent", "VolumeSnapshot"]),
    ("networking.istio.io", "v1beta1", ["DestinationRule", "Gateway", "ServiceEntry", "Sidecar", "VirtualService",
                                        "WorkloadEntry", "WorkloadGroup"]),
    ("security.istio.io", "v1beta1", ["AuthorizationPolicy", "PeerAuthentication", "RequestAuthentication"]),
    ("keda.sh", "v1alpha1", ["ClusterTriggerAuthentication", "ScaledJob", "ScaledObject", "TriggerAuthentication"]),
    ("velero.io", "v1", ["Backup", "BackupStorageLocation", "DeleteBackupRequest", "DownloadRequest",
                         "PodVolumeBackup", "PodVolumeRestore", "Restore", "Schedule", "ServerStatusRequest",
                         "VolumeSnapshotLocation"]),
]
# workload kinds a federation schedules (FederatedTypeConfig targets): the c3r units' GVKs and their shares
C3R_WORKLOADS = [(("apps", "v1", "Deployment"), 0.40), (("apps", "v1", "StatefulSet"), 0.15),
                 (("apps", "v1", "DaemonSet"), 0.10), (("batch", "v1", "Job"), 0.10),
                 (("batch", "v1", "CronJob"), 0.05), (("", "v1", "Service"), 0.10),
                 (("argoproj.io", "v1alpha1", "Rollout"), 0.05), (("apps.kruise.io", "v1alpha1", "CloneSet"), 0.05)]


def discovery_api_resources(rng: np.random.Generator, C: int, n_extra_crds: int = 40, p_operator: float = 0.9,
                            p_builtin: float = 1.0):
    """C clusters' ``APIResourceTypes`` shaped like updateClusterAPIResources' output (module comment above):
    the ~60 built-in resources (each with probability ``p_builtin``: 1 on real clusters), each operator's
    group with probability ``p_operator``, and ``n_extra_crds`` single-kind CRDs with probability
    ``p_operator`` each; Kind-sorted. About 150 entries per cluster (3 GVK words)."""
    def res(groups):
        out = []
        for g, v, kinds in groups:
            for k in kinds:
                out.append(T.APIResource(g, v, k, k.lower() + "s", "Namespaced"))
        return out

    builtin = res(_BUILTIN_API)
    ops = [res([grp]) for grp in _OPERATOR_API]
    extra = [T.APIResource(f"crd{i // 4}.example.com", "v1", f"Custom{i:02d}", f"custom{i:02d}s", "Namespaced")
             for i in range(n_extra_crds)]
    lists = []
    for _ in range(C):
        lst = list(builtin) if p_builtin >= 1.0 else [r for r, k in zip(builtin, rng.random(len(builtin)) < p_builtin) if k]
        for grp, keep in zip(ops, rng.random(len(ops)) < p_operator):
            if keep:
                lst.extend(grp)
        lst.extend(r for r, keep in zip(extra, rng.random(len(extra)) < p_operator) if keep)
        lst.sort(key=lambda r: r.kind)  # clusterstatus.go:262-264 (stable here, see module comment)
        lists.append(lst)
    return lists


def profile_for(config: str) -> F.Framework:
    """The plugin set each config is quoted on (BASELINE.json configs)."""
    if config in ("c2", "c3", "c3r", "c3p"):
        return F.Framework(F.EnabledPlugins(
            [F.APIResources, F.TaintToleration, F.ClusterResourcesFit, F.ClusterAffinity],
            [F.ClusterResourcesLeastAllocated], [F.MaxCluster], [F.ClusterCapacityWeight]))
    return F.Framework(F.default_enabled_plugins())


# ----------------------------------------------------------------- clusters
def gen_clusters(rng: np.random.Generator, C: int, n_keys=8, n_vals=8, n_int_keys=0, n_taints=16,
                 taints_per=(0, 3), p_gvk=1.0, gvks=GVKS[:1], scalars=False) -> List[T.FederatedCluster]:
    alloc_cpu = rng.integers(8_000, 4_000_001, C)
    alloc_mem = rng.integers(32 * GI, 16 * TI + 1, C, dtype=np.int64)
    fa = rng.random(C)
    fm = rng.random(C)
    taint_pool = [T.Taint(f"taint-{i % max(1, n_taints // 3)}", f"v{i}", EFFECTS[i % 3]) for i in range(n_taints)]
    out = []
    for c in range(C):
        labels = {}
        for k in range(n_keys):
            if rng.random() < 0.9:
                labels[f"key{k}"] = f"val{int(rng.integers(0, n_vals))}"
        for k in range(n_int_keys):
            if rng.random() < 0.9:
                labels[f"num{k}"] = str(int(rng.integers(0, 1000)))
        nt = int(rng.integers(taints_per[0], taints_per[1] + 1)) if n_taints else 0
        taints = [taint_pool[int(i)] for i in rng.choice(n_taints, size=min(nt, n_taints), replace=False)] if nt else []
        api = [T.APIResource(*g) for g in gvks if rng.random() < p_gvk]
        ac, am = int(alloc_cpu[c]), int(alloc_mem[c])
        vc, vm = int(ac * fa[c]), int(am * fm[c])
        alloc = {"cpu": f"{ac}m", "memory": str(am)}
        avail = {"cpu": f"{vc}m", "memory": str(vm)}
        if scalars:
            g = int(rng.integers(0, 9))
            alloc["example.com/gpu"] = str(g)
            avail["example.com/gpu"] = str(int(rng.integers(0, g + 1)))
        out.append(T.FederatedCluster(name=f"cluster-{c:05d}", labels=labels, taints=taints,
                                      api_resource_types=api, allocatable=alloc, available=avail))
    return out


def _tolerations(rng, n_taints, lo, hi, allow_wild=False):
    tols = []
    for _ in range(int(rng.integers(lo, hi + 1))):
        i = int(rng.integers(0, max(1, n_taints)))
        r = rng.random()
        if allow_wild and r < 0.05:
            tols.append(T.Toleration("", T.TOLERATION_OP_EXISTS, "", ""))
        elif r < 0.5:
            tols.append(T.Toleration(f"taint-{i % max(1, n_taints // 3)}", T.TOLERATION_OP_EQUAL, f"v{i}",
                                     EFFECTS[i % 3] if rng.random() < 0.7 else ""))
        else:
            tols.append(T.Toleration(f"taint-{i % max(1, n_taints // 3)}", T.TOLERATION_OP_EXISTS, "",
                                     EFFECTS[int(rng.integers(0, 3))] if rng.random() < 0.7 else ""))
    return tols


def _expr(rng, n_keys, n_vals, n_int_keys=0, all_ops=False, p_invalid=0.0):
    if p_invalid and rng.random() < p_invalid:
        bad = int(rng.integers(0, 4))
        if bad == 0:
            return T.ClusterSelectorRequirement("key0", T.OP_IN, ["invalid value: ___@#$%^"])
        if bad == 1:
            return T.ClusterSelectorRequirement("bad key/with/slashes", T.OP_EXISTS, None)
        if bad == 2:
            return T.ClusterSelectorRequirement("key1", "Bogus", ["val1"])
        return T.ClusterSelectorRequirement("key2", T.OP_IN, [])
    ops = [T.OP_IN, T.OP_NOT_IN, T.OP_EXISTS] + ([T.OP_DOES_NOT_EXIST, T.OP_GT, T.OP_LT] if all_ops else [])
    op = ops[int(rng.integers(0, len(ops)))]
    if op in (T.OP_GT, T.OP_LT) and n_int_keys:
        return T.ClusterSelectorRequirement(f"num{int(rng.integers(0, n_int_keys))}", op,
                                            [str(int(rng.integers(0, 1000)))])
    if op in (T.OP_GT, T.OP_LT):
        op = T.OP_IN
    key = f"key{int(rng.integers(0, n_keys))}"
    if op in (T.OP_EXISTS, T.OP_DOES_NOT_EXIST):
        return T.ClusterSelectorRequirement(key, op, None)
    nv = int(rng.integers(1, 4))
    return T.ClusterSelectorRequirement(key, op, [f"val{int(v)}" for v in rng.integers(0, n_vals, nv)])


# ------------------------------------------------------------------- units
def gen_units_c2(rng, W: int, n_keys=8, n_vals=8, n_taints=16, mode=T.SCHEDULING_MODE_DUPLICATE,
                 prefix="su") -> List[T.SchedulingUnit]:
    cpu = rng.integers(0, 64_001, W)
    mem = rng.integers(0, 256 * GI + 1, W, dtype=np.int64)
    maxc = rng.integers(1, 17, W)
    out = []
    for w in range(W):
        sel = None
        if rng.random() < 0.5:
            sel = {f"key{int(rng.integers(0, n_keys))}": f"val{int(rng.integers(0, n_vals))}"}
        exprs = [_expr(rng, n_keys, n_vals) for _ in range(int(rng.integers(1, 3)))]
        aff = T.Affinity(T.ClusterAffinity(required=T.ClusterSelector([T.ClusterSelectorTerm(exprs)])))
        out.append(T.SchedulingUnit(
            group="apps", version="v1", kind="Deployment", resource="deployments", namespace="default",
            name=f"{prefix}-{w}", desired_replicas=int(rng.integers(1, 101)),
            resource_request=T.Resource(int(cpu[w]), int(mem[w])), scheduling_mode=mode,
            cluster_selector=sel, affinity=aff, tolerations=_tolerations(rng, n_taints, 0, 3),
            max_clusters=int(maxc[w])))
    return out


def gen_units_c1(rng, W: int, clusters) -> List[T.SchedulingUnit]:
    names = [c.name for c in clusters]
    out = []
    for w in range(W):
        weights = None
        if w % 2 == 0:
            weights = {n: int(rng.integers(0, 11)) for n in names}
        out.append(T.SchedulingUnit(
            group="apps", version="v1", kind="Deployment", namespace="default", name=f"dep-{w}",
            desired_replicas=int(rng.integers(1, 101)), scheduling_mode=T.SCHEDULING_MODE_DIVIDE,
            avoid_disruption=True, weights=weights, tolerations=_tolerations(rng, 16, 0, 3),
            resource_request=T.Resource(int(rng.integers(0, 4001)), int(rng.integers(0, 8 * GI)))))
    return out


def gen_units_c4(rng, W: int, clusters) -> List[T.SchedulingUnit]:
    names = [c.name for c in clusters]
    C = len(names)
    out = []
    for w in range(W):
        k = int(rng.integers(8, 65))
        place = [names[int(i)] for i in rng.choice(C, size=min(k, C), replace=False)]
        weights = {n: int(rng.integers(0, 101)) for n in place} if rng.random() < 0.5 else None
        mins = {n: int(rng.integers(0, 6)) for n in place if rng.random() < 0.3}
        maxs = {n: int(rng.integers(0, 200)) for n in place if rng.random() < 0.3}
        caps = {n: int(rng.integers(0, 500)) for n in place if rng.random() < 0.2}
        cur = None
        if rng.random() < 0.25:
            cur = {n: (int(rng.integers(0, 300)) if rng.random() < 0.9 else None)
                   for n in place if rng.random() < 0.5}
        out.append(T.SchedulingUnit(
            group="apps", version="v1", kind="Deployment", namespace=f"ns{w % 7}", name=f"c4-{w}",
            desired_replicas=int(rng.integers(1, 10_001)), scheduling_mode=T.SCHEDULING_MODE_DIVIDE,
            avoid_disruption=bool(rng.random() < 0.5), cluster_names=set(place), weights=weights,
            min_replicas=mins or None, max_replicas=maxs or None, current_clusters=cur,
            auto_migration=T.AutoMigrationSpec(caps, bool(rng.random() < 0.5)) if caps else None,
            tolerations=_tolerations(rng, 16, 0, 3)))
    return out


def gen_units_c5(rng, W: int, clusters, n_keys=64, n_vals=16, n_int_keys=4, n_taints=256):
    names = [c.name for c in clusters]
    out = []
    for w in range(W):
        terms = []
        for _ in range(int(rng.integers(2, 9))):
            exprs = [_expr(rng, n_keys, n_vals, n_int_keys, all_ops=True, p_invalid=0.01)
                     for _ in range(int(rng.integers(2, 7)))]
            fields = None
            if rng.random() < 0.3:
                fields = [T.ClusterSelectorRequirement("metadata.name", T.OP_NOT_IN,
                                                       [names[int(rng.integers(0, len(names)))]])]
            terms.append(T.ClusterSelectorTerm(exprs, fields))
        prefs = [T.PreferredSchedulingTerm(int(rng.integers(1, 101)), T.ClusterSelectorTerm(
            [_expr(rng, n_keys, n_vals, n_int_keys, all_ops=True) for _ in range(int(rng.integers(1, 4)))]))
            for _ in range(int(rng.integers(2, 5)))]
        out.append(T.SchedulingUnit(
            group=GVKS[w % 8][0], version="v1", kind=GVKS[w % 8][2], namespace="default", name=f"c5-{w}",
            desired_replicas=int(rng.integers(1, 101)), scheduling_mode=T.SCHEDULING_MODE_DIVIDE
            if rng.random() < 0.5 else T.SCHEDULING_MODE_DUPLICATE,
            affinity=T.Affinity(T.ClusterAffinity(T.ClusterSelector(terms), prefs)),
            tolerations=_tolerations(rng, n_taints, 1, 8, allow_wild=True), max_clusters=int(rng.integers(1, 17)),
            resource_request=T.Resource(int(rng.integers(0, 64_001)), int(rng.integers(0, 256 * GI)))))
    return out


def make_config(config: str, scale: float = 1.0, seed: Optional[int] = None, W: Optional[int] = None,
                C: Optional[int] = None) -> Tuple[List[T.FederatedCluster], List[T.SchedulingUnit], F.Framework]:
    W0, C0 = SIZES[config]
    W = W if W is not None else max(1, int(W0 * scale))
    if C is None:
        C = C0 if config != "c5" else max(16, int(C0 * min(1.0, scale * 10)))
    rng = np.random.default_rng(SEEDS[config] if seed is None else seed)
    if config == "c1":
        cl = gen_clusters(rng, C, p_gvk=1.0)
        return cl, gen_units_c1(rng, W, cl), profile_for(config)
    if config in ("c2", "c3"):
        cl = gen_clusters(rng, C)
        return cl, gen_units_c2(rng, W), profile_for(config)
    if config in ("c3r", "c3p"):
        cl = gen_clusters(rng, C)
        for c, api in zip(cl, discovery_api_resources(np.random.default_rng([SEEDS[config], 0xA91]), C)):
            c.api_resource_types = api
        units = gen_units_c2(rng, W)
        if config == "c3p":  # over-committed / cordoned clusters, no ResourceRequest (bench.make_clusters)
            production_resources(cl, np.random.default_rng([SEEDS[config], 0x9E5]))
            for su in units:
                su.resource_request = T.Resource()
        r2 = np.random.default_rng([SEEDS[config], 0x6E7])
        gv = [g for g, _ in C3R_WORKLOADS]
        share = np.array([p for _, p in C3R_WORKLOADS])
        for su, i in zip(units, r2.choice(len(gv), size=W, p=share / share.sum())):
            su.group, su.version, su.kind = gv[i]
        return cl, units, profile_for(config)
    if config == "c4":
        cl = gen_clusters(rng, C)
        return cl, gen_units_c4(rng, W, cl), profile_for(config)
    if config == "c5":
        cl = gen_clusters(rng, C, n_keys=64, n_vals=16, n_int_keys=4, n_taints=256, taints_per=(4, 16), p_gvk=0.9,
                          gvks=GVKS)
        return cl, gen_units_c5(rng, W, cl), profile_for(config)
    raise KeyError(config)


# ------------------------------------------------------------------- fuzz
def widen_prefs(units, seed: int, share: float = 0.3):
    """Push some preference-map values of ``units`` (in place) past int32 — weights, min / max replicas,
    estimated capacities of 2^31 … 2^40 — so the packers choose the wide (i64) preference columns
    (KAD_BATCH_NARROW_PREFS off). Returns the units."""
    rng = np.random.default_rng(seed)
    for su in units:
        if rng.random() >= share:
            continue
        maps = [m for m in (su.weights, su.min_replicas, su.max_replicas,
                            su.auto_migration.estimated_capacity if su.auto_migration is not None else None) if m]
        for m in maps:
            for k in list(m):
                if rng.random() < 0.5 and m[k] is not None and m[k] >= 0:
                    m[k] = int(m[k]) + int(rng.integers(1 << 31, 1 << 40))
    return units


def gen_fuzz(seed: int, W: int = 60, C: Optional[int] = None, n_taints: int = 9):
    """Small batch hitting every branch: all operators, invalid requirements, nil/empty terms, fields,
    sticky, current clusters, scalars, NoExecute on scheduled clusters, ties, weights/min/max/caps.
    n_taints > 64 spreads the taint ids over several 64-bit words (SnapDev::TW > 1)."""
    rng = np.random.default_rng(seed)
    C = C if C is not None else int(rng.integers(1, 40))
    cl = gen_clusters(rng, C, n_keys=4, n_vals=3, n_int_keys=2, n_taints=n_taints,
                      taints_per=(0, 3) if n_taints <= 9 else (1, 12), p_gvk=0.8, gvks=GVKS[:3], scalars=True)
    # make scores tie-heavy: quantise resources on some clusters
    for c in cl:
        if rng.random() < 0.5:
            c.allocatable["cpu"] = "8"
            c.available["cpu"] = "4"
            c.allocatable["memory"] = "16Gi"
            c.available["memory"] = "8Gi"
        if rng.random() < 0.1:
            c.taints = c.taints + c.taints[:1]  # duplicate taint: PNS counts with multiplicity
        if rng.random() < 0.05:
            c.labels = None
    names = [c.name for c in cl] + ["ghost-cluster"]
    units = []
    for w in range(W):
        r = rng.random
        mode = T.SCHEDULING_MODE_DUPLICATE if r() < 0.4 else T.SCHEDULING_MODE_DIVIDE
        aff = None
        if r() < 0.8:
            req = None
            if r() < 0.7:
                terms = []
                for _ in range(int(rng.integers(0, 4))):
                    exprs = [_expr(rng, 5, 4, 3, all_ops=True, p_invalid=0.08) for _ in range(int(rng.integers(0, 3)))]
                    fields = None
                    if r() < 0.3:
                        fk = "metadata.name" if r() < 0.8 else "metadata.namespace"
                        op = [T.OP_IN, T.OP_NOT_IN, T.OP_EXISTS][int(rng.integers(0, 3))] if r() < 0.9 else T.OP_IN
                        vals = [names[int(rng.integers(0, len(names)))]] if r() < 0.9 else ["a", "b"]
                        fields = [T.ClusterSelectorRequirement(fk, op, vals)]
                    terms.append(T.ClusterSelectorTerm(exprs if (exprs or r() < 0.5) else None, fields))
                req = T.ClusterSelector(terms if (terms or r() < 0.5) else None)
            prefs = None
            if r() < 0.6:
                prefs = []
                for _ in range(int(rng.integers(0, 4))):
                    exprs = [_expr(rng, 5, 4, 3, all_ops=True, p_invalid=0.05) for _ in range(int(rng.integers(0, 3)))]
                    wgt = int(rng.integers(-20, 101)) if r() < 0.9 else 0
                    prefs.append(T.PreferredSchedulingTerm(wgt, T.ClusterSelectorTerm(exprs)))
            aff = T.Affinity(T.ClusterAffinity(req, prefs) if r() < 0.95 else None)
        sel = None
        if r() < 0.3:
            sel = {f"key{int(rng.integers(0, 5))}": f"val{int(rng.integers(0, 4))}" for _ in range(int(rng.integers(0, 3)))}
        place = None
        if r() < 0.3:
            place = {names[int(i)] for i in rng.integers(0, len(names), int(rng.integers(0, 6)))}
        cur = None
        if r() < 0.3:
            cur = {names[int(i)]: (int(rng.integers(0, 30)) if r() < 0.8 else None)
                   for i in rng.integers(0, len(names), int(rng.integers(0, 4)))}
        weights = None
        if r() < 0.4:
            weights = {names[int(i)]: int(rng.integers(0, 10)) for i in rng.integers(0, len(names), int(rng.integers(0, 6)))}
        mins = {names[int(i)]: int(rng.integers(0, 5)) for i in rng.integers(0, len(names), 2)} if r() < 0.3 else None
        maxs = {names[int(i)]: int(rng.integers(0, 8)) for i in rng.integers(0, len(names), 2)} if r() < 0.3 else None
        am = None
        if r() < 0.3:
            am = T.AutoMigrationSpec({names[int(i)]: int(rng.integers(-2, 6)) for i in rng.integers(0, len(names), 3)}
                                     if r() < 0.8 else None, bool(r() < 0.5))
        scal = None
        if r() < 0.2:
            scal = {"example.com/gpu": int(rng.integers(0, 4))}
            if r() < 0.3:
                scal["example.com/missing"] = int(rng.integers(0, 2))
        g = GVKS[int(rng.integers(0, 4))]
        units.append(T.SchedulingUnit(
            group=g[0], version=g[1], kind=g[2], namespace="ns" if r() < 0.7 else "", name=f"fz-{seed}-{w}",
            desired_replicas=(int(rng.integers(-1, 40)) if r() < 0.9 else None),
            resource_request=T.Resource(int(rng.integers(0, 5000)) if r() < 0.7 else 0,
                                        int(rng.integers(0, 20 * GI)) if r() < 0.7 else 0,
                                        int(rng.integers(0, 2)) if r() < 0.1 else 0, scal),
            current_clusters=cur, auto_migration=am, scheduling_mode=mode, sticky_cluster=bool(r() < 0.1),
            avoid_disruption=bool(r() < 0.5), cluster_selector=sel, cluster_names=place, affinity=aff,
            tolerations=(_tolerations(rng, n_taints, 0, 3 if n_taints <= 9 else 10, allow_wild=True)
                         if r() < 0.8 else None),
            max_clusters=(int(rng.integers(-1, 8)) if r() < 0.8 else None), min_replicas=mins, max_replicas=maxs,
            weights=weights))
    return cl, units


def with_discovery(clusters, units, seed: int, p_operator: float = 0.7, p_builtin: float = 0.9):
    """``clusters`` (in place) with discovery-shaped API-resource lists (:func:`discovery_api_resources`, with
    gaps in the built-ins too) and ``units`` (in place) over :data:`C3R_WORKLOADS`' kinds plus one kind no
    cluster serves: GVK ids past the first 64 (the snapshot interns ~150). Returns (clusters, units)."""
    rng = np.random.default_rng([seed, 0xD15C])
    for c, api in zip(clusters, discovery_api_resources(rng, len(clusters), p_operator=p_operator,
                                                        p_builtin=p_builtin)):
        c.api_resource_types = api
    kinds = [g for g, _ in C3R_WORKLOADS] + [("example.com", "v1", "NowhereServed")]
    for su, i in zip(units, rng.integers(0, len(kinds), len(units))):
        su.group, su.version, su.kind = kinds[int(i)]
    return clusters, units


FUZZ_PROFILES = [
    F.EnabledPlugins(),  # nothing: all clusters feasible, all selected
    None,  # default
    F.EnabledPlugins([F.ClusterAffinity, F.TaintToleration], [F.ClusterAffinity, F.TaintToleration],
                     [F.MaxCluster], [F.ClusterCapacityWeight]),
    F.EnabledPlugins([F.ClusterResourcesFit, F.APIResources, F.PlacementFilter],
                     [F.ClusterResourcesMostAllocated, F.ClusterResourcesBalancedAllocation],
                     [F.MaxCluster], [F.ClusterCapacityWeight]),
    F.EnabledPlugins([F.PlacementFilter], [F.ClusterResourcesLeastAllocated], [], [F.ClusterCapacityWeight]),
    F.EnabledPlugins([F.TaintToleration, F.ClusterResourcesFit], [F.TaintToleration,
                                                                  F.ClusterResourcesLeastAllocated,
                                                                  F.ClusterResourcesMostAllocated],
                     [F.MaxCluster], []),
]


def fuzz_framework(i: int) -> F.Framework:
    ep = FUZZ_PROFILES[i % len(FUZZ_PROFILES)]
    return F.Framework(ep if ep is not None else F.default_enabled_plugins())


# ------------------------------------------------------------ scheduling-trigger workload (§8(f) f4)
TRIGGER_SIZES = {"t1": (1000, 16), "t2": (100_000, 256)}


def _api_pool(n: int):
    base = [("apps", "v1", "Deployment", "deployments"), ("apps", "v1", "StatefulSet", "statefulsets"),
            ("apps", "v1", "DaemonSet", "daemonsets"), ("batch", "v1", "Job", "jobs"),
            ("batch", "v1", "CronJob", "cronjobs"), ("", "v1", "ConfigMap", "configmaps"),
            ("", "v1", "Secret", "secrets"), ("", "v1", "Service", "services"),
            ("networking.k8s.io", "v1", "Ingress", "ingresses")]
    out = [T.APIResource(g, v, k, p, "Namespaced") for g, v, k, p in base]
    i = 0
    while len(out) < n:
        out.append(T.APIResource(f"crd{i // 4}.example.com", f"v{1 + i % 2}", f"Kind{i}", f"kind{i}s",
                                 "Cluster" if i % 5 == 0 else "Namespaced"))
        i += 1
    return out[:n]


def gen_trigger_workload(rng: np.random.Generator, W: int, C: int, n_policies: int = 64, n_api: int = 64):
    """Joined clusters as the trigger hash sees them (labels, taints, ~n_api API resources each) and W
    federated Deployments: a policy out of ``n_policies`` (some with auto migration), replicas 1-100,
    10 % with scheduling annotations. Returns (type_config, clusters, objects, policies)."""
    from . import objects as O

    clusters = gen_clusters(rng, C)
    pool = _api_pool(n_api)
    for c in clusters:
        keep = rng.random(len(pool)) < 0.9
        api = [pool[i] for i in np.nonzero(keep)[0]]
        rng.shuffle(api)
        c.api_resource_types = api
    pols = [O.PropagationPolicy(f"policy-{i}", "default", int(rng.integers(1, 20)), O.PropagationPolicySpec(
        scheduling_mode=T.SCHEDULING_MODE_DIVIDE,
        auto_migration=O.AutoMigration() if i % 4 == 0 else None)) for i in range(n_policies)]
    ftc = O.FederatedTypeConfig("apps", "v1", "Deployment", "deployments", "Namespaced", "spec.replicas")
    objs, opols = [], []
    for w in range(W):
        p = pols[int(rng.integers(0, n_policies))]
        ann = {O.PROPAGATION_POLICY_NAME_LABEL: p.name}
        annotations = {"kubectl.kubernetes.io/last-applied-configuration": "{}"}
        r = rng.random()
        if r < 0.05:
            annotations[O.MAX_CLUSTERS_ANNOTATIONS] = str(int(rng.integers(1, 8)))
        elif r < 0.10:
            annotations[O.PLACEMENTS_ANNOTATIONS] = json.dumps(
                [{"cluster": clusters[int(rng.integers(0, C))].name, "preferences": {"weight": int(rng.integers(1, 9))}}])
        if p.spec.auto_migration is not None and rng.random() < 0.5:
            annotations[O.AUTO_MIGRATION_INFO_ANNOTATION] = json.dumps(
                {"estimatedCapacity": {clusters[int(rng.integers(0, C))].name: int(rng.integers(0, 50))}})
        objs.append({"apiVersion": "types.kubeadmiral.io/v1alpha1", "kind": "FederatedDeployment",
                     "metadata": {"name": f"app-{w}", "namespace": "default", "labels": ann,
                                  "annotations": annotations},
                     "spec": {"template": {"apiVersion": "apps/v1", "kind": "Deployment",
                                           "metadata": {"name": f"app-{w}", "namespace": "default"},
                                           "spec": {"replicas": int(rng.integers(1, 101))}}}})
        opols.append(p)
    return ftc, clusters, objs, opols


# ------------------------------------------------------- cluster update events
def mutate_clusters(rng: np.random.Generator, clusters: List[T.FederatedCluster], n_changed: int,
                    structural: bool = True) -> Tuple[List[T.FederatedCluster], List[int]]:
    """A cluster informer update: ``n_changed`` clusters get new status resources (the periodic status
    collection) and, with ``structural``, label values / taints / API resources drawn from what the other
    clusters already carry (so the snapshot vocabulary does not grow). Returns (new list, changed positions)."""
    import copy

    vals: Dict[str, list] = {}
    taints, apis = {}, {}
    for c in clusters:
        for k, v in (c.labels or {}).items():
            vals.setdefault(k, []).append(v)
        for t in c.taints:
            taints[(t.key, t.value, t.effect)] = t
        for r in c.api_resource_types:
            apis[(r.group, r.version, r.kind)] = r
    taint_pool, api_pool = list(taints.values()), list(apis.values())
    idx = sorted(int(i) for i in rng.choice(len(clusters), size=min(n_changed, len(clusters)), replace=False))
    out = list(clusters)
    for i in idx:
        c = copy.deepcopy(clusters[i])
        if c.allocatable and "cpu" in c.allocatable:
            ac = k8s.milli_value(k8s.quantity(c.allocatable["cpu"]))
            am = k8s.value(k8s.quantity(c.allocatable["memory"])) if "memory" in c.allocatable else 0
            c.available = dict(c.available or {}, cpu=f"{int(ac * rng.random())}m", memory=str(int(am * rng.random())))
            if "example.com/gpu" in c.allocatable:
                c.available["example.com/gpu"] = str(int(rng.integers(0, int(c.allocatable["example.com/gpu"]) + 1)))
        if structural:
            if c.labels and rng.random() < 0.5:
                k = sorted(c.labels)[int(rng.integers(0, len(c.labels)))]
                c.labels = dict(c.labels)
                c.labels[k] = vals[k][int(rng.integers(0, len(vals[k])))]
            if taint_pool and rng.random() < 0.4:
                nt = int(rng.integers(0, min(4, len(taint_pool)) + 1))
                c.taints = [taint_pool[int(j)] for j in rng.choice(len(taint_pool), size=nt, replace=False)]
            if api_pool and rng.random() < 0.3:
                c.api_resource_types = [r for r in api_pool if rng.random() < 0.8]
        out[i] = c
    return out, idx


# ------------------------------------------------------------ columnar generator (native packer input)
def gen_units_c2_columns(rng: np.random.Generator, W: int, n_keys=8, n_vals=8, n_taints=16,
                         mode=T.SCHEDULING_MODE_DUPLICATE, prefix="su", workloads=None):
    """The C2/C3 workload of :func:`gen_units_c2` (same distributions, its own random stream) generated
    directly as ``columns.SUColumns`` with numpy — the packer input a Go shim would hand over — so 1M-unit
    batches (C3) are generated in about a second instead of minutes of Python objects.

    ``workloads``: [((group, version, kind), share), ...] — each unit's GVK drawn with these shares (c3r:
    :data:`C3R_WORKLOADS`) after every other column, so the rest of the batch equals the one without it;
    default: every unit an apps/v1 Deployment."""
    from . import columns as CO

    st = CO.StringTable()
    sid = st.id
    key_ids = np.array([sid(f"key{k}") for k in range(n_keys)], np.int32)
    val_ids = np.array([sid(f"val{v}") for v in range(n_vals)], np.int32)
    op_ids = np.array([sid(o) for o in (T.OP_IN, T.OP_NOT_IN, T.OP_EXISTS)], np.int32)
    nt5 = max(1, n_taints // 3)
    tkey_ids = np.array([sid(f"taint-{i % nt5}") for i in range(max(1, n_taints))], np.int32)
    tval_ids = np.array([sid(f"v{i}") for i in range(max(1, n_taints))], np.int32)
    empty = sid("")
    eff_ids = np.array([sid(e) for e in EFFECTS], np.int32)
    equal_id, exists_id = sid(T.TOLERATION_OP_EQUAL), sid(T.TOLERATION_OP_EXISTS)
    g, v, k, ns = sid("apps"), sid("v1"), sid("Deployment"), sid("default")
    name0 = len(st._parts)
    for w in range(W):
        st._parts.append(f"{prefix}-{w}".encode())
    str_off, str_data = st.arrays()

    cols = {}
    cols["group"] = np.full(W, g, np.int32)
    cols["version"] = np.full(W, v, np.int32)
    cols["kind"] = np.full(W, k, np.int32)
    cols["namespace_"] = np.full(W, ns, np.int32)
    cols["name"] = np.arange(name0, name0 + W, dtype=np.int32)
    f = CO.SU_HAS_DESIRED | CO.SU_HAS_MAX_CLUSTERS | CO.SU_HAS_CLUSTER_AFFINITY | CO.SU_HAS_REQUIRED
    if mode == T.SCHEDULING_MODE_DUPLICATE:
        f |= CO.SU_DUPLICATE
    cols["flags"] = np.full(W, f, np.uint32)
    cols["req_cpu"] = rng.integers(0, 64_001, W).astype(np.int64)
    cols["req_mem"] = rng.integers(0, 256 * GI + 1, W, dtype=np.int64)
    cols["req_eph"] = np.zeros(W, np.int64)
    cols["max_clusters"] = rng.integers(1, 17, W).astype(np.int64)
    cols["desired"] = rng.integers(1, 101, W).astype(np.int64)
    # ClusterSelector: half the units, one entry
    has_sel = rng.random(W) < 0.5
    ns_ = int(has_sel.sum())
    cols["sel_off"] = CO._csr_off(has_sel.astype(np.int32))
    cols["sel_key"] = key_ids[rng.integers(0, n_keys, ns_)]
    cols["sel_value"] = val_ids[rng.integers(0, n_vals, ns_)]
    # one required term of 1-2 In / NotIn / Exists expressions
    n_expr = rng.integers(1, 3, W).astype(np.int32)
    R = int(n_expr.sum())
    cols["rterm_off"] = np.arange(W + 1, dtype=np.int32)
    rt_req = np.zeros(W, np.int32)
    rt_req[1:] = np.cumsum(n_expr)[:-1]
    cols["rt_req"] = rt_req
    cols["rt_n_expr"] = n_expr
    cols["rt_n_field"] = np.zeros(W, np.int32)
    op = rng.integers(0, 3, R)
    cols["rq_key"] = key_ids[rng.integers(0, n_keys, R)]
    cols["rq_op"] = op_ids[op]
    nv = np.where(op == 2, 0, rng.integers(1, 4, R)).astype(np.int32)
    cols["rq_val_off"] = CO._csr_off(nv)
    cols["rq_val"] = val_ids[rng.integers(0, n_vals, int(nv.sum()))]
    # tolerations: 0-3, half Equal (effect 70 %), half Exists (random effect 70 %)
    n_tol = rng.integers(0, 4, W).astype(np.int32)
    TT = int(n_tol.sum())
    cols["tol_off"] = CO._csr_off(n_tol)
    i = rng.integers(0, max(1, n_taints), TT)
    r = rng.random(TT)
    with_eff = rng.random(TT) < 0.7
    eq = r < 0.5
    cols["tol_key"] = tkey_ids[i]
    cols["tol_op"] = np.where(eq, equal_id, exists_id).astype(np.int32)
    cols["tol_value"] = np.where(eq, tval_ids[i], empty).astype(np.int32)
    eff = np.where(eq, eff_ids[i % 3], eff_ids[rng.integers(0, 3, TT)])
    cols["tol_effect"] = np.where(with_eff, eff, empty).astype(np.int32)
    zero_off = np.zeros(W + 1, np.int32)
    for grp in ("scalar", "pterm", "place", "cur", "wt", "min", "max", "cap"):
        cols[grp + "_off"] = zero_off
    for kname, dt in CO.FIELDS:
        if kname not in cols:
            cols[kname] = np.zeros(0, dt)
    if workloads:
        gvks = [wk for wk, _ in workloads]
        share = np.array([p for _, p in workloads], np.float64)
        pick = rng.choice(len(gvks), size=W, p=share / share.sum())
        # the string table already holds every unit name: new strings go after them
        ids = np.array([[st.id(x) for x in g] for g in gvks], np.int32)
        str_off, str_data = st.arrays()
        cols["group"], cols["version"], cols["kind"] = ids[pick, 0], ids[pick, 1], ids[pick, 2]
    return CO.SUColumns(W, str_off, str_data, cols)


def _tol_columns(rng, st, W: int, n_taints: int, lo: int, hi: int, allow_wild: bool = False):
    """Columns of :func:`_tolerations` (same distribution, vectorised): lo..hi tolerations per unit; 5 %
    wildcard (empty key, Exists) with ``allow_wild``; else half Equal (key/value of a pool taint, its effect
    70 %), half Exists (a pool key, a random effect 70 %)."""
    from . import columns as CO

    sid = st.id
    nt = max(1, n_taints)
    nt3 = max(1, n_taints // 3)
    tkey = np.array([sid(f"taint-{i % nt3}") for i in range(nt)], np.int32)
    tval = np.array([sid(f"v{i}") for i in range(nt)], np.int32)
    eff = np.array([sid(e) for e in EFFECTS], np.int32)
    empty, equal_id, exists_id = sid(""), sid(T.TOLERATION_OP_EQUAL), sid(T.TOLERATION_OP_EXISTS)
    n = rng.integers(lo, hi + 1, W).astype(np.int32)
    TT = int(n.sum())
    i = rng.integers(0, nt, TT)
    r = rng.random(TT)
    with_eff = rng.random(TT) < 0.7
    wild = (r < 0.05) if allow_wild else np.zeros(TT, bool)
    eq = ~wild & (r < 0.5)
    e = np.where(eq, eff[i % 3], eff[rng.integers(0, 3, TT)])
    return {"tol_off": CO._csr_off(n),
            "tol_key": np.where(wild, empty, tkey[i]).astype(np.int32),
            "tol_op": np.where(eq, equal_id, exists_id).astype(np.int32),
            "tol_value": np.where(eq, tval[i], empty).astype(np.int32),
            "tol_effect": np.where(wild | ~with_eff, empty, e).astype(np.int32)}


def _fill_columns(W: int, st, cols):
    from . import columns as CO

    zero_off = np.zeros(W + 1, np.int32)
    for grp in CO.CSR_GROUPS:
        cols.setdefault(grp + "_off", zero_off)
    cols.setdefault("rq_val_off", np.zeros(1, np.int32))  # no requirements: one offset
    for kname, dt in CO.FIELDS:
        if kname not in cols:
            cols[kname] = np.zeros(W if kname in ("desired", "max_clusters", "req_cpu", "req_mem", "req_eph")
                                   else 0, dt)
    str_off, str_data = st.arrays()
    return CO.SUColumns(W, str_off, str_data, cols)


def _names(st, W: int, prefix: str) -> np.ndarray:
    name0 = len(st._parts)
    for w in range(W):
        st._parts.append(f"{prefix}-{w}".encode())
    return np.arange(name0, name0 + W, dtype=np.int32)


def gen_units_c4_columns(rng: np.random.Generator, W: int, cluster_names, prefix="c4"):
    """The C4 replica-planner stress workload of :func:`gen_units_c4` (same distributions, its own random
    stream) as ``columns.SUColumns``: Divide units with ClusterNames of 8-64 distinct clusters (a random
    start and odd stride over the snapshot, distinct for C a power of two — else rejected and redrawn),
    static weights U{0..100} on half the units, MinReplicas U{0..5} / MaxReplicas U{0..199} on 30 % and
    EstimatedCapacity U{0..499} on 20 % of the entries (AutoMigration when any, KeepUnschedulable 50 %),
    CurrentClusters on 25 % of the units (half the entries, 10 % nil replicas), DesiredReplicas
    U{1..10 000}, AvoidDisruption 50 %, 0-3 tolerations."""
    from . import columns as CO

    C = len(cluster_names)
    st = CO.StringTable()
    sid = st.id
    cid = np.array([sid(n) for n in cluster_names], np.int32)
    g, v, k = sid("apps"), sid("v1"), sid("Deployment")
    nss = np.array([sid(f"ns{i}") for i in range(7)], np.int32)
    cols = {"group": np.full(W, g, np.int32), "version": np.full(W, v, np.int32), "kind": np.full(W, k, np.int32),
            "namespace_": nss[np.arange(W) % 7], "name": _names(st, W, prefix)}
    kk = np.minimum(rng.integers(8, 65, W), C).astype(np.int32)
    P = int(kk.sum())
    place_off = CO._csr_off(kk)
    unit_of = np.repeat(np.arange(W), kk)
    j = np.arange(P) - place_off[:-1][unit_of]
    start = rng.integers(0, C, W)
    if C & (C - 1) == 0:
        stride = (2 * rng.integers(0, max(1, C // 2), W) + 1) % C if C > 1 else np.zeros(W, np.int64)
        pos = (start[unit_of] + stride[unit_of] * j) % max(C, 1)
    else:  # consecutive clusters from a random start (distinct for k <= C)
        pos = (start[unit_of] + j) % C
    cols["place_off"] = place_off
    cols["place_name"] = cid[pos]
    has_w = rng.random(W) < 0.5
    wl = np.where(has_w, kk, 0).astype(np.int32)
    cols["wt_off"] = CO._csr_off(wl)
    sel_w = has_w[unit_of]
    cols["wt_name"] = cid[pos[sel_w]]
    cols["wt_val"] = rng.integers(0, 101, int(sel_w.sum())).astype(np.int64)

    def sub_map(p, lo, hi, grp):
        m = rng.random(P) < p
        cols[grp + "_off"] = CO._csr_off(np.bincount(unit_of[m], minlength=W).astype(np.int32))
        cols[grp + "_name"] = cid[pos[m]]
        cols[grp + "_val"] = rng.integers(lo, hi + 1, int(m.sum())).astype(np.int64)
        return m

    sub_map(0.3, 0, 5, "min")
    sub_map(0.3, 0, 199, "max")
    mc = sub_map(0.2, 0, 499, "cap")
    has_am = np.bincount(unit_of[mc], minlength=W) > 0
    has_cur = rng.random(W) < 0.25
    mcur = has_cur[unit_of] & (rng.random(P) < 0.5)
    cols["cur_off"] = CO._csr_off(np.bincount(unit_of[mcur], minlength=W).astype(np.int32))
    cols["cur_name"] = cid[pos[mcur]]
    ncur = int(mcur.sum())
    hr = rng.random(ncur) < 0.9
    cols["cur_rep"] = np.where(hr, rng.integers(0, 300, ncur), 0).astype(np.int64)
    cols["cur_has_rep"] = hr.astype(np.uint8)
    f = np.full(W, CO.SU_HAS_DESIRED, np.uint32)
    f |= np.where(rng.random(W) < 0.5, CO.SU_AVOID_DISRUPTION, 0).astype(np.uint32)
    f |= np.where(has_am, CO.SU_HAS_AUTO_MIGRATION, 0).astype(np.uint32)
    f |= np.where(has_am & (rng.random(W) < 0.5), CO.SU_KEEP_UNSCHED, 0).astype(np.uint32)
    cols["flags"] = f
    cols["desired"] = rng.integers(1, 10_001, W).astype(np.int64)
    cols.update(_tol_columns(rng, st, W, 16, 0, 3))
    return _fill_columns(W, st, cols)


def _expr_columns(rng, st, R: int, n_keys: int, n_vals: int, n_int_keys: int, p_invalid: float):
    """R requirements of :func:`_expr` (all_ops=True, vectorised): (rq_key, rq_op, per-requirement value
    counts, flat value ids)."""
    sid = st.id
    keys = np.array([sid(f"key{k}") for k in range(n_keys)], np.int32)
    ikeys = np.array([sid(f"num{k}") for k in range(max(1, n_int_keys))], np.int32)
    vals = np.array([sid(f"val{v}") for v in range(n_vals)], np.int32)
    nums = np.array([sid(str(i)) for i in range(1000)], np.int32)
    ops = np.array([sid(o) for o in (T.OP_IN, T.OP_NOT_IN, T.OP_EXISTS, T.OP_DOES_NOT_EXIST, T.OP_GT, T.OP_LT)],
                   np.int32)
    # the invalid forms of _expr: an invalid label value, an invalid key, an unknown operator, In with no value
    bad_key = np.array([sid("key0"), sid("bad key/with/slashes"), sid("key1"), sid("key2")], np.int32)
    bad_op = np.array([ops[0], ops[2], sid("Bogus"), ops[0]], np.int32)
    bad_nv = np.array([1, 0, 1, 0], np.int32)
    bad_v = np.array([sid("invalid value: ___@#$%^"), -1, sid("val1"), -1], np.int32)
    op = rng.integers(0, 6, R)
    if not n_int_keys:
        op = np.where(op >= 4, 0, op)
    rk = np.where(op >= 4, ikeys[rng.integers(0, max(1, n_int_keys), R)], keys[rng.integers(0, n_keys, R)])
    nv = np.where(op >= 4, 1, np.where(op >= 2, 0, rng.integers(1, 4, R)))
    rop = ops[op]
    inv = (rng.random(R) < p_invalid) if p_invalid else np.zeros(R, bool)
    bad = rng.integers(0, 4, R)
    rk = np.where(inv, bad_key[bad], rk).astype(np.int32)
    rop = np.where(inv, bad_op[bad], rop).astype(np.int32)
    nv = np.where(inv, bad_nv[bad], nv).astype(np.int32)
    owner = np.repeat(np.arange(R), nv)
    V = len(owner)
    rv = np.where(op[owner] >= 4, nums[rng.integers(0, 1000, V)], vals[rng.integers(0, n_vals, V)])
    rv = np.where(inv[owner], bad_v[bad[owner]], rv).astype(np.int32)
    return rk, rop, nv, rv


def _excl_in_group(lengths, group_first):
    """Offset of each item within its group: exclusive prefix of ``lengths`` minus that of the group's first
    item (``group_first[i]`` = index of item i's group's first item)."""
    excl = np.cumsum(lengths) - lengths
    return excl - excl[group_first]


def gen_units_c5_columns(rng: np.random.Generator, W: int, cluster_names, n_keys=64, n_vals=16, n_int_keys=4,
                         n_taints=256, prefix="c5"):
    """The C5 adversarial-filtering workload of :func:`gen_units_c5` (same distributions, its own random
    stream) as ``columns.SUColumns``: 2-8 required terms of 2-6 expressions over every operator (1 %
    invalid) with a metadata.name NotIn field on 30 % of the terms, 2-4 preferred terms of 1-3 expressions
    (weights U{1..100}), GVK = GVKS[w % 8], Divide / Duplicate 50/50, 1-8 tolerations over 256 taints
    (5 % wildcard), MaxClusters U{1..16}, requests cpu U[0, 64 000] milli, memory U[0, 256 GiB)."""
    from . import columns as CO

    C = len(cluster_names)
    st = CO.StringTable()
    sid = st.id
    cid = np.array([sid(n) for n in cluster_names], np.int32)
    gv = [(sid(g[0]), sid("v1"), sid(g[2])) for g in GVKS]
    gw = np.arange(W) % 8
    cols = {"group": np.array([gv[i][0] for i in range(8)], np.int32)[gw],
            "version": np.array([gv[i][1] for i in range(8)], np.int32)[gw],
            "kind": np.array([gv[i][2] for i in range(8)], np.int32)[gw],
            "namespace_": np.full(W, sid("default"), np.int32), "name": _names(st, W, prefix)}
    md_name, notin = sid("metadata.name"), sid(T.OP_NOT_IN)
    # required terms: 2-8 per unit, 2-6 expressions, 30 % with one metadata.name field
    nrt = rng.integers(2, 9, W).astype(np.int32)
    NT = int(nrt.sum())
    ne = rng.integers(2, 7, NT).astype(np.int32)
    nf = (rng.random(NT) < 0.3).astype(np.int32)
    # preferred terms: 2-4 per unit, 1-3 expressions
    npt = rng.integers(2, 5, W).astype(np.int32)
    NP = int(npt.sum())
    pne = rng.integers(1, 4, NP).astype(np.int32)
    # requirement table: unit by unit, its required terms (exprs then fields), then its preferred terms
    rt_unit = np.repeat(np.arange(W), nrt)
    pt_unit = np.repeat(np.arange(W), npt)
    per_rt = ne + nf
    req_per_unit = np.bincount(rt_unit, weights=per_rt, minlength=W).astype(np.int64) + \
        np.bincount(pt_unit, weights=pne, minlength=W).astype(np.int64)
    unit_base = np.zeros(W + 1, np.int64)
    unit_base[1:] = np.cumsum(req_per_unit)
    R = int(unit_base[-1])
    rterm_off, pterm_off = CO._csr_off(nrt), CO._csr_off(npt)
    rt_total = np.bincount(rt_unit, weights=per_rt, minlength=W).astype(np.int64)
    rt_req = (unit_base[:-1][rt_unit] + _excl_in_group(per_rt, rterm_off[:-1][rt_unit])).astype(np.int32)
    pt_req = (unit_base[:-1][pt_unit] + rt_total[pt_unit] +
              _excl_in_group(pne, pterm_off[:-1][pt_unit])).astype(np.int32)
    # which requirement slots are fields (one per term with nf, after its expressions)
    is_field = np.zeros(R, bool)
    is_field[(rt_req + ne)[nf == 1]] = True
    is_pref = np.zeros(R, bool)
    pref_slots = np.repeat(pt_req.astype(np.int64), pne) + _excl_in_group(
        np.ones(int(pne.sum()), np.int64), np.repeat(np.cumsum(pne) - pne, pne))
    is_pref[pref_slots] = True
    # expressions: required ones with 1 % invalid, preferred ones all valid
    rk = np.zeros(R, np.int32)
    rop = np.zeros(R, np.int32)
    nv = np.zeros(R, np.int32)
    out_v = []
    for mask, p_inv in ((~is_field & ~is_pref, 0.01), (is_pref, 0.0)):
        idx = np.nonzero(mask)[0]
        k_, o_, n_, v_ = _expr_columns(rng, st, len(idx), n_keys, n_vals, n_int_keys, p_inv)
        rk[idx], rop[idx], nv[idx] = k_, o_, n_
        out_v.append((idx, n_, v_))
    fidx = np.nonzero(is_field)[0]
    rk[fidx], rop[fidx], nv[fidx] = md_name, notin, 1
    out_v.append((fidx, np.ones(len(fidx), np.int32), cid[rng.integers(0, C, len(fidx))]))
    val_off = CO._csr_off(nv)
    rq_val = np.zeros(int(val_off[-1]), np.int32)
    for idx, n_, v_ in out_v:
        if len(v_):
            dst = np.repeat(val_off[:-1][idx].astype(np.int64), n_) + _excl_in_group(
                np.ones(int(n_.sum()), np.int64), np.repeat(np.cumsum(n_) - n_, n_))
            rq_val[dst] = v_
    cols.update({"rq_key": rk, "rq_op": rop, "rq_val_off": val_off, "rq_val": rq_val,
                 "rterm_off": rterm_off, "rt_req": rt_req, "rt_n_expr": ne, "rt_n_field": nf,
                 "pterm_off": pterm_off, "pt_weight": rng.integers(1, 101, NP).astype(np.int32),
                 "pt_req": pt_req, "pt_n_expr": pne})
    f = np.full(W, CO.SU_HAS_DESIRED | CO.SU_HAS_MAX_CLUSTERS | CO.SU_HAS_CLUSTER_AFFINITY | CO.SU_HAS_REQUIRED,
                np.uint32)
    f |= np.where(rng.random(W) < 0.5, 0, CO.SU_DUPLICATE).astype(np.uint32)
    cols["flags"] = f
    cols["desired"] = rng.integers(1, 101, W).astype(np.int64)
    cols["max_clusters"] = rng.integers(1, 17, W).astype(np.int64)
    cols["req_cpu"] = rng.integers(0, 64_001, W).astype(np.int64)
    cols["req_mem"] = rng.integers(0, 256 * GI, W, dtype=np.int64)
    cols.update(_tol_columns(rng, st, W, n_taints, 1, 8, allow_wild=True))
    return _fill_columns(W, st, cols)


# ------------------------------------------------------- result application (§8 f3)
def gen_result_objects(rng: np.random.Generator, W: int, names: List[str], replicas_path: str = "/spec/replicas"):
    """W federated objects whose placements / overrides exercise every branch of applySchedulingResult's
    result-dependent half: the scheduler's placement present or not (other controllers' placements beside
    it, a second scheduler entry after the first), clusters from the snapshot, unknown names and duplicates,
    an empty cluster list; replicas-path override patches with integral, fractional and non-numeric values,
    other paths, other controllers, clusters outside the snapshot."""
    from . import objects as O

    sched = O.PREFIXED_GLOBAL_SCHEDULER_NAME
    pool = list(names) + ["ghost-a", "ghost-b"]
    out = []
    for w in range(W):
        r = rng.random
        pls = []
        if r() < 0.3:
            pls.append({"controller": "other-controller", "placement": {"clusters": [{"name": pool[0]}]}})
        if r() < 0.75:
            k = int(rng.integers(0, 6))
            cl = [{"name": pool[int(i)]} for i in rng.integers(0, len(pool) if r() < 0.3 else len(names), k)]
            pls.append({"controller": sched, "placement": {"clusters": cl} if (cl or r() < 0.5) else {}})
            if r() < 0.1:
                pls.append({"controller": sched, "placement": {"clusters": [{"name": pool[1]}]}})
        ovs = []
        if r() < 0.6:
            clusters = []
            for c in sorted({pool[int(i)] for i in rng.integers(0, len(pool) if r() < 0.2 else len(names),
                                                                 int(rng.integers(0, 6)))}):
                paths = []
                if r() < 0.2:
                    paths.append({"path": "/spec/template/spec/containers/0/image", "value": "nginx"})
                if r() < 0.85:
                    v = r()
                    val = float(rng.integers(0, 40)) if v < 0.8 else (float(rng.integers(0, 40)) + 0.5 if v < 0.9
                                                                      else str(int(rng.integers(0, 40))))
                    paths.append({"path": replicas_path, "value": val})
                clusters.append({"clusterName": c, "paths": paths})
            ovs.append({"controller": sched, "clusters": clusters})
        if r() < 0.2:
            ovs.append({"controller": "other-controller", "clusters": [{"clusterName": pool[0], "paths": [
                {"path": replicas_path, "value": 7.0}]}]})
        obj = {"apiVersion": "types.kubeadmiral.io/v1alpha1", "kind": "FederatedDeployment",
               "metadata": {"name": f"obj-{w}", "namespace": "default"}, "spec": {"template": {}}}
        if pls or r() < 0.5:
            obj["spec"]["placements"] = pls
        if ovs:
            obj["spec"]["overrides"] = ovs
        out.append(obj)
    return out


def gen_override_policies(seed: int, clusters, n_policies: int = 40, max_rules: int = 6, n_keys: int = 4,
                          n_vals: int = 3, n_int_keys: int = 2, p_invalid: float = 0.03, namespaces=("ns",)):
    """(Cluster)OverridePolicies over the label vocabulary of :func:`gen_clusters` / :func:`gen_fuzz` clusters:
    0..max_rules rules each, targets mixing nil, names (some unknown), selectors, affinity terms with fields and
    empty terms, and — with probability ``p_invalid`` per part — invalid selectors, expressions, fields and
    patch values. Draws from its own generator, so no other seeded workload changes."""
    from . import overrides as OV

    rng = np.random.default_rng([seed, 0x6F7672])
    r = rng.random
    names = [c.name for c in clusters] + ["ghost-cluster"]
    values = [b"1", b'"s"', b'{"k": [1, true, null]}', b"[1.5, 2]", b""]
    pols = []
    for i in range(n_policies):
        rules = []
        for _ in range(int(rng.integers(0, max_rules + 1))):
            tc = None
            if r() < 0.85:
                tc = OV.TargetClusters()
                if r() < 0.35:
                    k = int(rng.integers(0, min(len(names), 8) + 1))
                    tc.clusters = [names[int(j)] for j in rng.integers(0, len(names), k)]
                if r() < 0.35:
                    tc.cluster_selector = {f"key{int(rng.integers(0, n_keys))}": f"val{int(rng.integers(0, n_vals))}"
                                           for _ in range(int(rng.integers(0, 3)))}
                    if r() < p_invalid:
                        tc.cluster_selector["bad key/with/slashes" if r() < 0.5 else "key0"] = "invalid value: @"
                if r() < 0.5:
                    terms = []
                    for _ in range(int(rng.integers(0, 4))):
                        exprs = [_expr(rng, n_keys, n_vals, n_int_keys, all_ops=True, p_invalid=p_invalid)
                                 for _ in range(int(rng.integers(0, 3)))]
                        fields = None
                        if r() < 0.3:
                            op = T.OP_EXISTS if r() < p_invalid else (T.OP_IN if r() < 0.6 else T.OP_NOT_IN)
                            fields = [T.ClusterSelectorRequirement("metadata.name", op,
                                                                   [names[int(rng.integers(0, len(names)))]])]
                        terms.append(T.ClusterSelectorTerm(exprs or None, fields))
                    tc.cluster_affinity = terms
            patches = [OV.JsonPatchOverrider(["add", "replace", "remove"][int(rng.integers(0, 3))],
                                             f"/spec/f{int(rng.integers(0, 6))}",
                                             b"{broken" if r() < p_invalid else values[int(rng.integers(0, len(values)))])
                       for _ in range(int(rng.integers(0, 3)))]
            rules.append(OV.OverrideRule(tc, patches))
        ns = None if i % 2 == 0 else namespaces[int(rng.integers(0, len(namespaces)))]
        pols.append(OV.OverridePolicy(f"op-{seed}-{i}", ns, rules))
    return pols


# ------------------------------------------------------------ follower scheduling (kad_follower_union)
def gen_followers(seed: int, lead_off, lead_cluster, n_ids: int, per_leader: float = 2.0, max_leaders: int = 3,
                  changed: float = 0.01):
    """A synthetic follower set over leaders whose cluster sets are the CSR ``lead_off`` / ``lead_cluster``
    (ids below ``n_ids``): ``per_leader`` followers per leader on average, each following 1..``max_leaders``
    leaders drawn near one another (objects of one namespace). A follower's current placement is the union of
    its leaders' sets — in another order, so unchanged — except for a fraction ``changed`` of them, which lack
    one cluster of it or, where the union is empty, hold one stale cluster. Returns kad_follower_union's
    follower arrays (fol_off, fol_leader, cur_off, cur_cluster, cur_has) and the changed mask."""
    rng = np.random.default_rng([seed, 0xF011])
    lead_off = np.asarray(lead_off, np.int64)
    lead_cluster = np.asarray(lead_cluster, np.int32)
    L = len(lead_off) - 1
    F = int(round(L * per_leader))
    n = rng.integers(1, max_leaders + 1, F).astype(np.int32)
    fol_off = np.zeros(F + 1, np.int32)
    fol_off[1:] = np.cumsum(n)
    base = rng.integers(0, max(1, L), F)
    owner = np.repeat(np.arange(F), n)
    fol_leader = ((base[owner] + rng.integers(0, 8, len(owner))) % max(1, L)).astype(np.int32)
    stale = rng.random(F) < changed
    cur_off = np.zeros(F + 1, np.int32)
    cur, has = [], np.ones(F, np.uint8)
    for i in range(F):
        ls = fol_leader[fol_off[i]:fol_off[i + 1]]
        u = np.unique(np.concatenate([lead_cluster[lead_off[ld]:lead_off[ld + 1]] for ld in ls])) if L else \
            np.zeros(0, np.int32)
        if stale[i]:
            u = u[1:] if len(u) else np.array([int(rng.integers(0, n_ids))], np.int32)
        elif len(u) == 0:
            has[i] = 0
        cur.append(u[::-1])
        cur_off[i + 1] = cur_off[i] + len(u)
    cur_cluster = np.concatenate(cur).astype(np.int32) if cur else np.zeros(0, np.int32)
    return (fol_off, fol_leader, cur_off, cur_cluster, has), stale


# ------------------------------------------------------------ auto migration (kad_migrate_estimate)
MIGRATION_NOW_NS = 1_760_000_000 * 10**9  # a fixed "now" (October 2025) for seeded workloads


def gen_migration(seed: int, W: int, C: int, ready_share: float = 0.9, max_segments: int = 5, replicas=(1, 100),
                  unschedulable: float = 0.3, changed: float = 0.05, extra_ids: int = 0, now_ns: int = MIGRATION_NOW_NS,
                  thresholds_s=(30, 60, 300)):
    """A synthetic auto-migration batch as kad_migrate_estimate's arrays: ``W`` objects with a threshold out
    of ``thresholds_s`` (seconds), each on 1..``max_segments`` member clusters out of ``C + extra_ids`` ids. A share
    ``ready_share`` of the segments has total == ready (KAD_MIG_SEG_SKIP, no pods; 1 % of them a failed listing
    with backoff); the others hold about as many pods as desired replicas (``replicas``, the range of the
    synthetic Deployments), a share ``unschedulable`` of them unschedulable since a time within two minutes
    around the threshold, 5 % deleting, 1 % of the unschedulable ones without a transition time. The existing
    annotation is the batch's own result except for a share ``changed`` of the objects, which lack its first
    entry or, where it is empty, hold one stale entry. Returns (arrays — the keyword arguments of
    Context.migrate_estimate —, the changed mask)."""
    from . import automigration as AM

    rng = np.random.default_rng([seed, 0xA070])
    n_ids = C + extra_ids
    max_segments = max(1, min(max_segments, n_ids))
    nseg = rng.integers(1, max_segments + 1, W)
    so = np.zeros(W + 1, np.int64)
    so[1:] = np.cumsum(nseg)
    S = int(so[-1])
    owner = np.repeat(np.arange(W), nseg)
    k = np.arange(S) - so[owner]
    step = rng.integers(1, max(1, n_ids // max_segments) + 1, W)
    start = (rng.random(W) * (n_ids - step * (nseg - 1))).astype(np.int64)
    seg_cluster = (start[owner] + k * step[owner]).astype(np.int32)
    desired = rng.integers(replicas[0], replicas[1] + 1, S)
    skip = rng.random(S) < ready_share
    flags = np.where(skip, AM.SEG_SKIP, 0).astype(np.uint8)
    flags[skip & (rng.random(S) < 0.01)] |= AM.SEG_BACKOFF
    npods = np.where(skip, 0, np.maximum(0, desired + rng.integers(-2, 3, S)))
    po = np.zeros(S + 1, np.int64)
    po[1:] = np.cumsum(npods)
    P = int(po[-1])
    thr = rng.choice(np.array(thresholds_s, np.int64) * 10**9, W)
    pod_obj = owner[np.repeat(np.arange(S), npods)]
    pf = np.where(rng.random(P) < unschedulable, AM.POD_UNSCHED, 0).astype(np.uint8)
    pf[rng.random(P) < 0.05] |= AM.POD_DELETING
    pf[(rng.random(P) < 0.01) & ((pf & AM.POD_UNSCHED) != 0)] |= AM.POD_TZERO
    pt = now_ns - thr[pod_obj] + rng.integers(-60 * 10**9, 60 * 10**9 + 1, P)
    pt[(pf & AM.POD_TZERO) != 0] = 0
    a = dict(n_ids=n_ids, now_ns=int(now_ns), obj_seg_off=so.astype(np.int32), obj_threshold_ns=thr,
             seg_cluster=seg_cluster, seg_desired=desired.astype(np.int64), seg_flags=flags, seg_pod_off=po,
             pod_t_ns=pt.astype(np.int64), pod_flags=pf, old_off=np.zeros(W + 1, np.int32),
             old_cluster=np.zeros(0, np.int32), old_cap=np.zeros(0, np.int64))
    r = AM.migrate_numpy(**a)
    written = r["cap"] >= 0
    stale = rng.random(W) < changed
    first = np.zeros(S, bool)
    wi = np.nonzero(written)[0]
    if len(wi):
        first[wi[np.r_[True, owner[wi][1:] != owner[wi][:-1]]]] = True
    keep = written & ~(first & stale[owner])
    n_old = np.bincount(owner[keep], minlength=W)
    fake = stale & (r["n_written"] == 0)  # nothing to drop: one stale entry instead
    oc, ov, oo = seg_cluster[keep], r["cap"][keep], owner[keep]
    if fake.any():
        fo = np.nonzero(fake)[0]
        oc = np.concatenate([oc, seg_cluster[so[fo]]])
        ov = np.concatenate([ov, np.full(len(fo), 7, np.int64)])
        oo = np.concatenate([oo, fo])
        order = np.argsort(oo, kind="stable")
        oc, ov = oc[order], ov[order]
        n_old = n_old + fake
    a["old_off"] = np.r_[0, np.cumsum(n_old)].astype(np.int32)
    a["old_cluster"], a["old_cap"] = oc.astype(np.int32), ov.astype(np.int64)
    return a, stale


def migration_objects(a: dict, names, type_config=None):
    """The batch of :func:`gen_migration` as the controller sees it: federated objects with the threshold and
    the existing annotation, per object the (cluster name, member Deployment) pairs, and per pair the pod dicts
    (a PodListError for a backoff segment). ``names``: cluster names by id (``a['n_ids']`` of them). For small
    batches: tests. Returns (type_config, objs, cluster_objs, pods)."""
    import datetime

    from . import automigration as AM
    from . import objects as O

    ftc = type_config or O.FederatedTypeConfig("apps", "v1", "Deployment", "deployments", "Namespaced", "spec.replicas",
                                               "status.replicas", "status.readyReplicas")
    epoch = datetime.datetime(1970, 1, 1)

    def rfc3339(ns: int) -> str:
        t = epoch + datetime.timedelta(microseconds=ns // 1000)
        return t.strftime("%Y-%m-%dT%H:%M:%S") + f".{ns % 10**9:09d}Z"

    objs, cobjs, pods = [], [], []
    for i in range(len(a["obj_threshold_ns"])):
        ann = {O.POD_UNSCHEDULABLE_THRESHOLD_ANNOTATION: O.duration_string(int(a["obj_threshold_ns"][i]))}
        q0, q1 = int(a["old_off"][i]), int(a["old_off"][i + 1])
        if q1 > q0:
            ann[O.AUTO_MIGRATION_INFO_ANNOTATION] = AM.marshal_info(
                {names[int(a["old_cluster"][q])]: int(a["old_cap"][q]) for q in range(q0, q1)})
        objs.append({"apiVersion": "types.kubeadmiral.io/v1alpha1", "kind": "FederatedDeployment",
                     "metadata": {"name": f"app-{i}", "namespace": "default", "annotations": ann},
                     "spec": {"template": {"apiVersion": "apps/v1", "kind": "Deployment",
                                           "metadata": {"name": f"app-{i}", "namespace": "default"},
                                           "spec": {"replicas": 1}}}})
        co, pl = [], []
        for s in range(int(a["obj_seg_off"][i]), int(a["obj_seg_off"][i + 1])):
            sf, desired = int(a["seg_flags"][s]), int(a["seg_desired"][s])
            p0, p1 = int(a["seg_pod_off"][s]), int(a["seg_pod_off"][s + 1])
            skip = bool(sf & AM.SEG_SKIP) and not sf & AM.SEG_BACKOFF
            status = {"replicas": desired, "readyReplicas": desired if skip else max(0, desired - 1)}
            co.append((names[int(a["seg_cluster"][s])],
                       {"apiVersion": "apps/v1", "kind": "Deployment", "spec": {"replicas": desired}, "status": status}))
            if sf & AM.SEG_BACKOFF:
                pl.append(AM.PodListError("listing failed", needs_backoff=True))
                continue
            seg = []
            for p in range(p0, p1):
                f = int(a["pod_flags"][p])
                cond = {"type": "PodScheduled", "status": "True"}
                if f & AM.POD_UNSCHED:
                    cond = {"type": "PodScheduled", "status": "False", "reason": "Unschedulable"}
                if not f & AM.POD_TZERO:
                    cond["lastTransitionTime"] = rfc3339(int(a["pod_t_ns"][p]))
                pod = {"metadata": {"name": f"app-{i}-{p}"}, "status": {"conditions": [cond]}}
                if f & AM.POD_DELETING:
                    pod["metadata"]["deletionTimestamp"] = rfc3339(int(a["now_ns"]))
                seg.append(pod)
            pl.append(seg)
        objs[-1]["spec"]["template"]["spec"]["replicas"] = int(a["seg_desired"][int(a["obj_seg_off"][i])])
        cobjs.append(co)
        pods.append(pl)
    return ftc, objs, cobjs, pods


# ------------------------------------------------------------ cluster status (kad_cluster_resources)
CSTAT_NAMES = ("cpu", "memory", "ephemeral-storage", "example.com/gpu")
CSTAT_SCALES = (3, 0, 0, 0)  # cpu in milli, the others in units


def gen_cluster_status(seed: int, K: int, nodes_median: float = 300.0, sigma: float = 1.3, pods_per_node: float = 30.0,
                       max_nodes: int = 20000, schedulable: float = 0.95, terminal: float = 0.1):
    """Seeded nodes and pods of ``K`` member clusters as kad_cluster_resources' arrays, sizes skewed: nodes per
    cluster log-normal around ``nodes_median`` (``sigma``; clipped to [3, ``max_nodes``]: tens to thousands), pods
    about ``pods_per_node`` times as many. Every node lists cpu, memory and ephemeral-storage, one in ten a GPU
    resource; a share ``schedulable`` of the nodes is schedulable. A pod has 1-3 containers requesting cpu and
    memory, one in ten an init container, one in twenty an overhead, one in fifty a GPU; a share ``terminal`` is
    Succeeded / Failed. Returns (arrays — the keyword arguments of Context.cluster_resources —, CSTAT_NAMES,
    CSTAT_SCALES)."""
    rng = np.random.default_rng([seed, 0xC57A])
    nn = np.clip(rng.lognormal(np.log(nodes_median), sigma, K), 3, max_nodes).astype(np.int64)
    npod = np.maximum(0, (nn * pods_per_node * rng.uniform(0.6, 1.4, K)).astype(np.int64))
    cn = np.zeros(K + 1, np.int64)
    cn[1:] = np.cumsum(nn)
    cp = np.zeros(K + 1, np.int64)
    cp[1:] = np.cumsum(npod)
    N, P = int(cn[-1]), int(cp[-1])
    # nodes: entries ascend by resource id; slot 3 (the GPU) on one node in ten
    gpu = rng.random(N) < 0.1
    ncnt = np.stack([np.ones(N, np.int8)] * 3 + [gpu.astype(np.int8)], axis=1)
    nent_res = np.repeat(np.tile(np.arange(4, dtype=np.uint8), N), ncnt.ravel())
    ne = np.zeros(N + 1, np.int64)
    ne[1:] = np.cumsum(ncnt.sum(axis=1, dtype=np.int64))
    cores = rng.choice(np.array([4, 8, 16, 32, 64, 96, 128], np.int64), N)
    per_node = np.stack([cores * 1000 - rng.integers(0, 500, N), cores * (4 << 30), rng.integers(100, 2000, N) << 30,
                         np.full(N, 8, np.int64)], axis=1)
    nent_val = per_node.ravel()[ncnt.ravel() > 0]
    node_flags = np.where(rng.random(N) < schedulable, 1, 0).astype(np.uint8)
    # pods: nine (resource, kind) slots in ascending order over cpu, memory and the GPU
    ncont = rng.integers(1, 4, P).astype(np.int8)
    init = (rng.random(P) < 0.1).astype(np.int8)
    ovh = (rng.random(P) < 0.05).astype(np.int8)
    pgpu = (rng.random(P) < 0.02).astype(np.int8)
    zero = np.zeros(P, np.int8)
    pcnt = np.stack([ncont, init, ovh, ncont, init, ovh, pgpu, zero, zero], axis=1)
    slot = np.repeat(np.tile(np.arange(9, dtype=np.uint8), P), pcnt.ravel())
    pe = np.zeros(P + 1, np.int64)
    pe[1:] = np.cumsum(pcnt.sum(axis=1, dtype=np.int64))
    pent_res = np.array([0, 0, 0, 1, 1, 1, 3, 3, 3], np.uint8)[slot]
    pent_kind = (slot % 3).astype(np.uint8)
    EP = len(slot)
    pent_val = np.where(pent_res == 0, rng.integers(10, 500, EP),
                        np.where(pent_res == 1, rng.integers(32, 2048, EP) << 20, 1)).astype(np.int64)
    pod_flags = np.where(rng.random(P) < terminal, 1, 0).astype(np.uint8)
    a = dict(n_res=4, cl_node_off=cn, node_flags=node_flags, node_ent_off=ne, nent_res=nent_res,
             nent_val=nent_val.astype(np.int64), cl_pod_off=cp, pod_flags=pod_flags, pod_ent_off=pe, pent_res=pent_res,
             pent_kind=pent_kind, pent_val=pent_val)
    return a, CSTAT_NAMES, CSTAT_SCALES


def cluster_status_objects(a: dict, names=CSTAT_NAMES, scales=CSTAT_SCALES):
    """The batch of :func:`gen_cluster_status` as the controller sees it: per cluster the node dicts (allocatable
    with a ``pods`` count; the unschedulable ones cordoned, tainted NoSchedule / NoExecute or not Ready in turn)
    and the pod dicts (containers, init containers, overhead, phase). For small batches: tests. Returns
    (cluster_nodes, cluster_pods)."""
    suffix = {0: "", 3: "m", 6: "u", 9: "n"}

    def text(r: int, v: int) -> str:
        return f"{int(v)}{suffix[scales[r]]}"

    cluster_nodes, cluster_pods = [], []
    for k in range(len(a["cl_node_off"]) - 1):
        nodes = []
        for n in range(int(a["cl_node_off"][k]), int(a["cl_node_off"][k + 1])):
            alloc = {"pods": "110"}
            for e in range(int(a["node_ent_off"][n]), int(a["node_ent_off"][n + 1])):
                alloc[names[int(a["nent_res"][e])]] = text(int(a["nent_res"][e]), a["nent_val"][e])
            node = {"metadata": {"name": f"node-{k}-{n}"}, "spec": {},
                    "status": {"allocatable": alloc, "conditions": [{"type": "Ready", "status": "True"}]}}
            if not a["node_flags"][n] & 1:
                how = n % 4
                if how == 0:
                    node["spec"]["unschedulable"] = True
                elif how in (1, 2):
                    node["spec"]["taints"] = [{"key": "maintenance", "effect": ("NoSchedule", "NoExecute")[how - 1]}]
                else:
                    node["status"]["conditions"] = [{"type": "Ready", "status": "Unknown"}]
            elif n % 7 == 0:
                node["spec"]["taints"] = [{"key": "spot", "effect": "PreferNoSchedule"}]
            nodes.append(node)
        pods = []
        for p in range(int(a["cl_pod_off"][k]), int(a["cl_pod_off"][k + 1])):
            by_kind = ({}, {}, {})  # kind → resource → the values in order
            for e in range(int(a["pod_ent_off"][p]), int(a["pod_ent_off"][p + 1])):
                by_kind[int(a["pent_kind"][e])].setdefault(int(a["pent_res"][e]), []).append(int(a["pent_val"][e]))

            def containers(m):
                return [{"name": f"c{j}", "resources": {"requests": {names[r]: text(r, v[j]) for r, v in m.items()
                                                                     if j < len(v)}}}
                        for j in range(max((len(v) for v in m.values()), default=0))]

            spec = {"containers": containers(by_kind[0])}
            if by_kind[1]:
                spec["initContainers"] = containers(by_kind[1])
            if by_kind[2]:
                spec["overhead"] = {names[r]: text(r, sum(v)) for r, v in by_kind[2].items()}
            phase = ("Succeeded", "Failed")[p % 2] if a["pod_flags"][p] & 1 else "Running"
            pods.append({"metadata": {"name": f"pod-{k}-{p}"}, "spec": spec, "status": {"phase": phase}})
        cluster_nodes.append(nodes)
        cluster_pods.append(pods)
    return cluster_nodes, cluster_pods


SAGG_BASE_TIME = 1_700_000_000  # Unix seconds


def gen_status_aggregation(seed: int, kind: int, W: int, C: int, place_off=None, place_cluster=None, max_clusters: int = 5,
                           nil_share: float = 0.02, stale_share: float = 0.05, duplicate_share: float = 0.0005,
                           changed: float = 0.05):
    """A synthetic status-aggregation batch as kad_status_aggregate's arrays: ``W`` source objects of ``kind``
    (statusagg.DEPLOYMENT / JOB), one segment per placed member cluster. The placements are a scheduled batch's
    (``place_off[W + 1]`` / ``place_cluster``: the results' CSR) or, without one, 1..``max_clusters`` clusters an
    object; a share ``duplicate_share`` of the objects are Duplicate-mode workloads on every one of the ``C``
    clusters. Members have partly ready replicas (Deployment) or are running, completed or failed (Job), a share
    ``nil_share`` has a nil status, a share ``stale_share`` a synced generation behind the observed one. The old
    status is the batch's own result except for a share ``changed`` of the objects. Returns (arrays — the keyword
    arguments of Context.status_aggregate —, seg_cluster: the member cluster of every segment)."""
    from . import statusagg as SA

    rng = np.random.default_rng([seed, kind, 0x5A66])
    if place_off is None:
        nseg = rng.integers(1, max(1, min(max_clusters, C)) + 1, W)
        first = (rng.random(W) * (C - nseg + 1)).astype(np.int64)
    else:
        nseg = np.diff(np.asarray(place_off, np.int64))
        first = None
    dup = rng.random(W) < duplicate_share
    nseg = np.where(dup, C, nseg)
    off = np.zeros(W + 1, np.int64)
    off[1:] = np.cumsum(nseg)
    S = int(off[-1])
    owner = np.repeat(np.arange(W), nseg)
    k = np.arange(S) - off[owner]
    if first is not None:
        seg_cluster = np.where(dup[owner], k, first[owner] + k).astype(np.int32)
    else:
        src = np.asarray(place_off, np.int64)[owner] + k
        pc = np.asarray(place_cluster, np.int64)
        seg_cluster = np.where(dup[owner], k, pc[np.minimum(src, max(0, len(pc) - 1))] if len(pc) else k).astype(np.int32)
    nil = rng.random(S) < nil_share
    obj_flags = np.where(rng.random(W) < 0.9, SA.OBJ_UPTODATE, 0).astype(np.uint8)
    a = dict(kind=kind, obj_seg_off=off.astype(np.int32), obj_flags=obj_flags)
    if kind == SA.DEPLOYMENT:
        replicas = rng.integers(1, 101, S)
        ready = (replicas * rng.uniform(0.5, 1.0, S)).astype(np.int64)
        updated = np.maximum(ready, (replicas * rng.uniform(0.7, 1.0, S)).astype(np.int64))
        a["seg_vals"] = np.where(nil, 0, np.stack([replicas, updated, ready, ready, replicas - ready])).astype(np.int32)
        gen = rng.integers(1, 20, S)
        a["seg_observed"] = np.where(nil, 0, gen).astype(np.int64)
        a["seg_synced"] = np.where(nil, 0, np.where(rng.random(S) < stale_share, gen + 1, gen)).astype(np.int64)
        a["seg_flags"] = np.where(nil, SA.SEG_NIL, SA.SEG_SYNCED).astype(np.uint8)
        a["obj_generation"] = rng.integers(2, 50, W).astype(np.int64)
        a["obj_observed"] = a["obj_generation"] - (rng.random(W) < 0.2)
        a["old_vals"] = np.zeros((6, W), np.int64)
    else:
        cls = rng.random(S)
        start = SAGG_BASE_TIME - rng.integers(0, 86400, S)
        f = np.where(rng.random(S) < 0.97, SA.SEG_START, 0) | np.where(cls < 0.5, SA.SEG_DONE, np.where(cls < 0.6, SA.SEG_FAILED, 0))
        a["seg_flags"] = np.where(nil, SA.SEG_NIL, f).astype(np.uint8)
        a["seg_start"] = np.where((a["seg_flags"] & SA.SEG_START) != 0, start, 0).astype(np.int64)
        a["seg_done"] = np.where((a["seg_flags"] & SA.SEG_DONE) != 0, start + rng.integers(1, 7200, S), 0).astype(np.int64)
        done = (a["seg_flags"] & SA.SEG_DONE) != 0
        a["seg_vals"] = np.where(nil, 0, np.stack([np.where(done, 0, rng.integers(0, 4, S)), np.where(done, rng.integers(1, 9, S), 0),
                                                   rng.integers(0, 2, S)])).astype(np.int32)
        a["old_vals"] = np.zeros((5, W), np.int64)
    r = SA.sagg_numpy(**a)
    nv = len(a["seg_vals"])
    a["old_vals"][:nv] = r["sums"]
    if kind == SA.DEPLOYMENT:
        a["old_vals"][5] = r["observed"]
        a["obj_observed"] = r["observed"].copy()  # one field of the source: its status.observedGeneration
    else:
        a["old_vals"][3] = r["start_min"]
        a["old_vals"][4] = np.where((r["finished"] != 0) & (r["n_failed"] == 0), r["done_max"], SA.NO_DONE)
    a["old_vals"][0, rng.random(W) < changed] += 1
    return a, seg_cluster


def status_aggregation_objects(a: dict, seg_cluster, names):
    """The batch of :func:`gen_status_aggregation` as the controller sees it: per object the source object, its
    federated object (template in step with the source, so that IsResourcePropagated holds where the object is
    UPTODATE) and the member objects by cluster name (``names``: id → name). For small batches: tests. Returns
    (sources, fed_objects, cluster_objs)."""
    from . import statusagg as SA

    kind = a["kind"]
    off = a["obj_seg_off"]
    sources, feds, members = [], [], []
    for o in range(len(a["obj_flags"])):
        old = a["old_vals"][:, o]
        if kind == SA.DEPLOYMENT:
            status = {k: float(v) for k, v in zip(SA.DEP_FIELDS + ("observedGeneration",), old) if v}
            src = {"apiVersion": "apps/v1", "kind": "Deployment",
                   "metadata": {"name": f"d{o}", "namespace": "default", "generation": int(a["obj_generation"][o])},
                   "spec": {"replicas": 3}, "status": status}
        else:
            status = {k: int(v) for k, v in zip(SA.JOB_FIELDS, old) if v}
            if old[3] != SA.NO_START:
                status["startTime"] = SA.format_time(int(old[3]))
            if old[4] != SA.NO_DONE:
                status["completionTime"] = SA.format_time(int(old[4]))
            src = {"apiVersion": "batch/v1", "kind": "Job", "metadata": {"name": f"j{o}", "namespace": "default", "generation": 1},
                   "spec": {"parallelism": 2}, "status": status}
        utd = bool(a["obj_flags"][o] & SA.OBJ_UPTODATE)
        clusters, objs = [], {}
        for s in range(int(off[o]), int(off[o + 1])):
            name, f = names[int(seg_cluster[s])], int(a["seg_flags"][s])
            vals = [int(v) for v in a["seg_vals"][:, s]]
            if f & SA.SEG_NIL:
                st = None
            elif kind == SA.DEPLOYMENT:
                st = dict(zip(SA.DEP_FIELDS, vals), observedGeneration=int(a["seg_observed"][s]))
            else:
                st = dict(zip(SA.JOB_FIELDS, vals))
                if f & SA.SEG_START:
                    st["startTime"] = SA.format_time(int(a["seg_start"][s]))
                if f & SA.SEG_DONE:
                    st["completionTime"] = SA.format_time(int(a["seg_done"][s]))
                if f & SA.SEG_FAILED:
                    st["conditions"] = [{"type": "Failed", "status": "True"}]
            objs[name] = {"kind": src["kind"], "metadata": {"name": src["metadata"]["name"], "generation": 1}, "status": st}
            if kind == SA.JOB or f & SA.SEG_SYNCED:
                clusters.append({"name": name, "status": "OK",
                                 "generation": int(a["seg_synced"][s]) if kind == SA.DEPLOYMENT else 1})
        template = {k: v for k, v in src.items() if k != "status"}
        fed = {"metadata": {"name": src["metadata"]["name"], "generation": 4,
                            "annotations": {SA.OBSERVED_ANNOTATION_KEYS: "|", SA.OBSERVED_LABEL_KEYS: "|",
                                            SA.TEMPLATE_MERGE_PATCH: '{"status":null}'}},
               "spec": {"template": template}, "status": {"syncedGeneration": 4 if utd else 3, "clusters": clusters}}
        sources.append(src)
        feds.append(fed)
        members.append(objs)
    return sources, feds, members


ROLLOUT_FENCEPOSTS = ((0, 25), (25, 0), (25, 25), (10, 5))  # the template's (maxSurge %, maxUnavailable %)


def gen_rollout(seed: int, W: int, min_targets: int = 1, max_targets: int = 15, unchanged: float = 0.6,
                updated: float = 0.5, deviation: float = 0.1):
    """A synthetic rollout-planning batch as kad_rollout_plan's arrays (the keyword arguments of
    Context.rollout_plan): ``W`` federated Deployments in the middle of a rollout, each on ``min_targets`` ..
    ``max_targets`` member clusters (uniform; mean 8 by default). The template's fenceposts are one of
    ROLLOUT_FENCEPOSTS as percentages of the desired total, resolved as the reference resolves them (surge up,
    unavailable down, both zero: unavailable 1). A share ``unchanged`` of the targets keeps its size, the others are
    to grow or shrink by up to a third; a share ``updated`` already runs the new template, with a new replica set
    somewhere between empty and complete; a share ``deviation`` has one or two pods more or less than its spec, or
    not available. Every member object exists and none is to delete."""
    rng = np.random.default_rng([seed, 0x726F])
    n = rng.integers(min_targets, max_targets + 1, W)
    off = np.zeros(W + 1, np.int64)
    off[1:] = np.cumsum(n)
    T = int(off[-1])
    owner = np.repeat(np.arange(W), n)
    desired = rng.integers(0, 61, T)
    keep = rng.random(T) < unchanged
    delta = (desired * rng.uniform(-0.33, 0.33, T)).astype(np.int64)
    replicas = np.where(keep, desired, np.maximum(desired + delta, 0))
    upd = rng.random(T) < updated
    progress = rng.random(T)
    new = np.where(upd, np.where(progress < 0.4, replicas, (replicas * progress).astype(np.int64)), replicas)
    new_avail = np.where(upd, np.maximum(new - rng.integers(0, 3, T), 0), new)
    dev = rng.random(T) < deviation
    actual = np.maximum(replicas + np.where(dev, rng.integers(-1, 3, T), 0), 0)
    available = np.maximum(np.minimum(actual, replicas) - np.where(dev, rng.integers(0, 3, T), 0), 0)
    total = np.bincount(owner, weights=desired, minlength=W).astype(np.int64)
    fp = np.array(ROLLOUT_FENCEPOSTS, np.int64)[rng.integers(0, len(ROLLOUT_FENCEPOSTS), W)]
    p_ms = -((-fp[:, 0] * total) // 100)
    p_mu = (fp[:, 1] * total) // 100
    p_mu = np.where((p_ms == 0) & (p_mu == 0), 1, p_mu)
    # a member runs with what an earlier plan gave it: a share of the template's fenceposts
    share = rng.uniform(0.0, 0.6, T)
    ms = np.where(upd, (p_ms[owner] * share).astype(np.int64), 0)
    mu = np.where(upd, (p_mu[owner] * share).astype(np.int64), 0)
    mu = np.where((ms == 0) & (mu == 0), 1, mu)
    vals = np.stack([replicas, actual, available, np.where(upd, new, 0), np.where(upd, new_avail, 0), new, new_avail,
                     ms, mu, desired]).astype(np.int32)
    return dict(obj_tgt_off=off.astype(np.int32), obj_max_surge=p_ms.astype(np.int32),
                obj_max_unavailable=p_mu.astype(np.int32), obj_replicas=total.astype(np.int32),
                obj_flags=np.zeros(W, np.uint8), tgt_vals=vals, tgt_flags=np.where(upd, 3, 2).astype(np.uint8))


def rollout_objects(a, names):
    """The objects behind a :func:`gen_rollout` batch, for the object-level path: per object the federated Deployment
    (template, replicas overrides, current-revision annotation), its member Deployments by cluster name (an object's
    k-th target is on ``names[k]``, which must be sorted) and the selected clusters."""
    off = np.asarray(a["obj_tgt_off"], np.int64)
    v = np.asarray(a["tgt_vals"], np.int64)
    feds, members, selected = [], [], []
    for o in range(len(off) - 1):
        lo, hi = int(off[o]), int(off[o + 1])
        strategy = {"rollingUpdate": {"maxSurge": int(a["obj_max_surge"][o]), "maxUnavailable": int(a["obj_max_unavailable"][o])}}
        feds.append({"apiVersion": "types.kubeadmiral.io/v1alpha1", "kind": "FederatedDeployment",
                     "metadata": {"name": f"dp-{o}", "namespace": "default",
                                  "annotations": {"kubeadmiral.io/current-revision": "rev-new"}},
                     "spec": {"template": {"spec": {"replicas": 1, "strategy": strategy}},
                              "overrides": [{"controller": "kubeadmiral.io/global-scheduler", "clusters": [
                                  {"clusterName": names[i - lo], "patches": [{"path": "/spec/replicas", "value": float(v[9, i])}]}
                                  for i in range(lo, hi)]}]}})
        objs = {}
        for i in range(lo, hi):
            updated = bool(int(a["tgt_flags"][i]) & 1)
            objs[names[i - lo]] = {
                "apiVersion": "apps/v1", "kind": "Deployment",
                "metadata": {"name": f"dp-{o}", "namespace": "default", "annotations": {
                    "kubeadmiral.io/current-revision": "rev-new" if updated else "rev-old",
                    "latestreplicaset.kubeadmiral.io/name": f"dp-{o}-rs", "latestreplicaset.kubeadmiral.io/replicas": str(int(v[5, i])),
                    "latestreplicaset.kubeadmiral.io/available-replicas": str(int(v[6, i]))}},
                "spec": {"replicas": int(v[0, i]),
                         "strategy": {"rollingUpdate": {"maxSurge": int(v[7, i]), "maxUnavailable": int(v[8, i])}}},
                "status": {"replicas": int(v[1, i]), "availableReplicas": int(v[2, i])}}
        feds[-1]["spec"]["template"]["spec"]["replicas"] = 1
        members.append(objs)
        selected.append(set(objs))
    return feds, members, selected



def gen_dispatch(seed: int, W: int, C: int, placed: int = 5, observed: float = 0.8, healthy: float = 0.9):
    """A synthetic sync-dispatch batch as kad_dispatch_plan's arrays (the keyword arguments of
    Context.dispatch_plan): ``W`` federated objects over ``C`` joined clusters, each placed on ``placed`` - 2 ..
    ``placed`` + 2 clusters (uniform, as unsorted ids with the odd duplicate; 2 % of the entries name a cluster that
    is not joined). A share ``observed`` of the objects is in its steady state — the informers hold the member
    object in every placed cluster — the others in a uniform part of them; one object in ten is also held by a
    cluster it has left. 3 % of the lookups failed, 5 % of the member objects are being deleted, 10 % were adopted.
    A share ``healthy`` of the clusters is ready and carries the finalizer, the others draw the four flags at
    random. A quarter of the objects lie in one of up to 64 federated namespaces whose placements cover 85 % of the
    clusters, 3 % in a namespace that is not federated, 1 % have a placement that does not unmarshal; one in ten
    orphans all, one in ten the adopted."""
    rng = np.random.default_rng([seed, 0x6469])
    cluster_flags = np.where(rng.random(C) < healthy, 1 | 8, rng.integers(0, 16, C)).astype(np.uint8)
    n_pl = rng.integers(max(placed - 2, 0), placed + 3, W)
    pl_off = np.zeros(W + 1, np.int64)
    pl_off[1:] = np.cumsum(n_pl)
    P = int(pl_off[-1])
    owner = np.repeat(np.arange(W), n_pl)
    pl_cluster = rng.integers(0, C, P)
    rank = np.arange(P) - pl_off[owner]
    held = np.where(rng.random(W) < observed, n_pl, (rng.random(W) * (n_pl + 1)).astype(np.int64))
    pl_cluster = np.where(rng.random(P) < 0.02, -1, pl_cluster)
    seen = (rank < held[owner]) & (pl_cluster >= 0)
    stray = np.flatnonzero(rng.random(W) < 0.1)
    keys = np.unique(np.concatenate((owner[seen] * C + pl_cluster[seen], stray * C + rng.integers(0, C, len(stray)))))
    ob_owner, ob_cluster = keys // C, keys % C
    B = len(keys)
    u = rng.random(B)
    ob_flags = np.where(u < 0.03, 8, np.where(u < 0.08, 1 | 2, np.where(u < 0.18, 1 | 4, 1))).astype(np.uint8)
    ob_off = np.zeros(W + 1, np.int64)
    ob_off[1:] = np.cumsum(np.bincount(ob_owner, minlength=W))
    N = max(1, min(64, W // 8))
    rows = [np.where(rng.random(C) < 0.02, -1, rng.permutation(C))[:max(1, int(C * 0.85))] for _ in range(N)]
    ns_off = np.zeros(N + 1, np.int64)
    ns_off[1:] = np.cumsum([len(r) for r in rows])
    u = rng.random(W)
    obj_ns = np.where(u < 0.25, rng.integers(0, N, W), np.where(u < 0.28, -2, -1))
    u = rng.random(W)
    obj_flags = (np.where(u < 0.1, 2, np.where(u < 0.2, 4, 0)) | (rng.random(W) < 0.01)).astype(np.uint8)
    return dict(cluster_flags=cluster_flags, obj_flags=obj_flags, obj_ns=obj_ns.astype(np.int32),
                obj_pl_off=pl_off.astype(np.int32), pl_cluster=pl_cluster.astype(np.int32),
                ns_pl_off=ns_off.astype(np.int32), ns_cluster=np.concatenate(rows).astype(np.int32),
                obj_ob_off=ob_off.astype(np.int32), ob_cluster=ob_cluster.astype(np.int32), ob_flags=ob_flags,
                out_off=pl_off + ob_off)


def gen_deletion(seed: int, W: int, C: int, observed: int = 10, healthy: float = 1.0, adopted: float = 0.1):
    """A synthetic sync-deletion batch as kad_deletion_finish's arrays (the keyword arguments of
    Context.deletion_finish; those of Context.deletion_plan are ``DELETION_PLAN_KEYS`` of them): ``W`` terminating
    objects over ``C`` joined clusters, each held by ``observed`` - 2 .. ``observed`` + 2 clusters (uniform), except
    that one object in five is on its second pass and held by none. 2 % of the lookups failed, 20 % of the member
    objects are already being deleted, a share ``adopted`` was adopted. A share ``healthy`` of the clusters is ready,
    at both listings independently. 85 % of the objects carry the finalizer and delete, 5 % orphan all, 5 % orphan the
    adopted, 3 % have no federated object, 2 % no finalizer. 1 % of the operations fail, 0.5 % of the objects time
    out in either Wait(); every object has check rows on 0 to 2 clusters (an answer each, uniform)."""
    rng = np.random.default_rng([seed, 0x64656C])
    cluster_flags = np.where(rng.random(C) < healthy, 1 | 8, rng.integers(0, 8, C) * 2).astype(np.uint8)
    chk_cluster_flags = np.where(rng.random(C) < healthy, 1 | 8, rng.integers(0, 8, C) * 2).astype(np.uint8)
    u = rng.random(W)
    obj_flags = np.select([u < 0.85, u < 0.90, u < 0.95, u < 0.98], [1, 1 | 2, 1 | 4, 8], 0).astype(np.uint8)

    def rows(n_per):
        off = np.zeros(W + 1, np.int64)
        off[1:] = np.cumsum(n_per)
        owner = np.repeat(np.arange(W), n_per)
        keys = np.unique(owner * C + rng.integers(0, C, len(owner)))  # (a duplicate draw: one entry fewer)
        off[1:] = np.cumsum(np.bincount(keys // C, minlength=W))
        return off, keys % C

    n_ob = np.where(rng.random(W) < 0.2, 0, rng.integers(max(observed - 2, 0), observed + 3, W))
    ob_off, ob_cluster = rows(np.minimum(n_ob, C))
    B = len(ob_cluster)
    u = rng.random(B)
    ob_flags = np.where(u < 0.02, 8, np.where(u < 0.22, 1 | 2, 1) | np.where(rng.random(B) < adopted, 4, 0)).astype(np.uint8)
    chk_off, chk_cluster = rows(np.minimum(rng.integers(0, 3, W), C))
    K = len(chk_cluster)
    return dict(cluster_flags=cluster_flags, obj_flags=obj_flags, obj_ob_off=ob_off.astype(np.int32),
                ob_cluster=ob_cluster.astype(np.int32), ob_flags=ob_flags, op_ok=(rng.random(B) >= 0.01).astype(np.uint8),
                obj_wait=((rng.random(W) < 0.005) * 1 + (rng.random(W) < 0.005) * 2).astype(np.uint8),
                chk_off=chk_off.astype(np.int32), chk_cluster=chk_cluster.astype(np.int32),
                chk_flags=(1 << rng.integers(0, 4, K)).astype(np.uint8), chk_cluster_flags=chk_cluster_flags)


DELETION_PLAN_KEYS = ("cluster_flags", "obj_flags", "obj_ob_off", "ob_cluster", "ob_flags")


def gen_sync_finish(seed: int, W: int, C: int, touched: int, steady: float = 0.8):
    """A synthetic sync-completion batch as kad_sync_finish's arrays (the arguments of Context.sync_finish, the four
    scalars included): ``W`` federated objects over ``C`` joined clusters, each with ``touched`` dispatcher records
    on ascending distinct clusters (a random start and stride). A share ``steady`` of the objects is in its steady
    state: every record is an update that timed out into OK with the stored generation version, the stored
    PropagatedVersion and ``status.clusters`` say the same and the condition is True, so nothing is to be written;
    the others have one failed update in ten, a stored version list that lacks every third cluster, and a stored status that lacks its last cluster. Versions are interned
    as ``gen:1`` .. ``gen:8`` and ``rv:1``; the selected clusters are the records' clusters."""
    rng = np.random.default_rng([seed, 0x73796e])
    touched = min(touched, C)
    stride = np.maximum(1, rng.integers(1, max(2, C // max(touched, 1) + 1), W))
    start = (rng.random(W) * (C - (touched - 1) * stride)).astype(np.int64) if touched else np.zeros(W, np.int64)
    cl = (start[:, None] + np.arange(touched)[None, :] * stride[:, None]).astype(np.int32)  # [W, touched] ascending
    ok = rng.random(W) < steady
    ver = rng.integers(1, 10, (W, touched)).astype(np.int32)  # ids 1..8 gen:k, 9 rv:1
    failed = (~ok[:, None]) & (rng.random((W, touched)) < 0.1)
    ent_status = np.where(failed, 9, 21).astype(np.uint8)  # UpdateFailed / UpdateTimedOut
    ent_version = np.where(failed, 0, ver).astype(np.int32)
    off = (np.arange(W + 1) * touched).astype(np.int32)
    # the stored versions: all of them (steady), or without every third and with two untouched clusters in front
    keep_v = ok[:, None] | (np.arange(touched)[None, :] % 3 != 0)
    oldv_n = keep_v.sum(1)
    oldv_off = np.concatenate(([0], np.cumsum(oldv_n))).astype(np.int32)
    keep_s = ok[:, None] | (np.arange(touched)[None, :] < touched - 1)
    olds_off = np.concatenate(([0], np.cumsum(keep_s.sum(1)))).astype(np.int32)
    gen = np.concatenate(([0], np.arange(1, 9), [0])).astype(np.int64)
    flags = np.where(ok, 1 | 2 | 64 | 128, 1 | 2 | 16 | 64 | 128).astype(np.uint16)
    ne, nv = np.full(W, touched, np.int64), oldv_n.astype(np.int64)
    return {"n_clusters": C, "n_reasons": 3, "reason_check_clusters": 1, "reason_ns_not_federated": 2,
            "obj_flags": flags, "reason_in": np.zeros(W, np.int32), "cond_reason": np.zeros(W, np.int32),
            "sel_off": off, "sel_cluster": cl.reshape(-1), "ent_off": off, "ent_cluster": cl.reshape(-1),
            "ent_status": ent_status.reshape(-1), "ent_version": ent_version.reshape(-1),
            "oldv_off": oldv_off, "oldv_cluster": cl[keep_v], "oldv_version": ver[keep_v],
            "olds_off": olds_off, "olds_cluster": cl[keep_s], "olds_status": np.ones(int(keep_s.sum()), np.uint8),
            "olds_gen": gen[ver[keep_s]], "ver_gen": gen,
            "ver_flags": np.array([0] + [3] * 8 + [1], np.uint8),
            "ver_off": np.concatenate(([0], np.cumsum(ne + nv))).astype(np.int64),
            "st_off": np.concatenate(([0], np.cumsum(ne))).astype(np.int64)}


def gen_monitor_events(seed: int, n_objects: int = 40, n_clusters: int = 6, rounds: int = 4, kinds=("FederatedDeployment", "FederatedJob"),
                       t0_ns: int = 1_700_000_000_000_000_000, max_list: Optional[int] = None):
    """Seeded monitor events (monitor.py's event dicts): ``rounds`` lists of (now_ns, events) over a pool of
    ``n_objects`` keys of ``kinds``. Every branch of MonitorSubController.reconcile turns up: absent and deleted
    objects, missing / unparsable / fractional syncSuccessTimestamp, lastGeneration and lastSyncSuccessGeneration
    equal, different or zero-padded, status absent, clusterStatus entries without a name or a generation, member
    objects without one, member lists equal to the fed list, to the previous one, or neither; keys repeat within a
    round."""
    import random
    from datetime import datetime, timezone

    rng = random.Random(seed)
    max_list = n_clusters if max_list is None else max_list

    def stamp(ns: int) -> str:
        s, f = divmod(ns, 10 ** 9)
        base = datetime.fromtimestamp(s, timezone.utc).strftime("%Y-%m-%dT%H:%M:%S")
        return base + (("." + ("%09d" % f).rstrip("0")) if f else "") + "Z"

    keys = [f"{rng.choice(kinds)}/ns{j % 3}/obj{j}" for j in range(n_objects)]
    gens = {k: rng.randrange(1, 9) for k in keys}
    prev: dict = {}
    out = []
    now = t0_ns
    for _ in range(rounds):
        now += rng.randrange(1, 40 * 60) * 10 ** 9 + rng.randrange(10 ** 9)
        events = []
        for _ in range(rng.randrange(n_objects // 2, 2 * n_objects)):
            k = rng.choice(keys)
            r = rng.random()
            if r < 0.06:
                events.append(dict(key=k, obj=None, status_enabled=True, status=None, members=[]))
                continue
            if rng.random() < 0.3:
                gens[k] += 1
            g = gens[k]
            ann = {}
            r = rng.random()
            if r < 0.6:
                ann["syncSuccessTimestamp"] = stamp(now - rng.randrange(0, 3 * 3600 * 10 ** 9))
            elif r < 0.7:
                ann["syncSuccessTimestamp"] = rng.choice(["yesterday", "2023-13-01T00:00:00Z", ""])
            r = rng.random()
            if r < 0.8:
                ann["lastGeneration"] = rng.choice([str(g), str(g), str(g - 1), "0%d" % g])
            if rng.random() < 0.7:
                ann["lastSyncSuccessGeneration"] = rng.choice([str(g), str(g), str(g - 1)])
            meta = dict(generation=g, annotations=ann)
            if rng.random() < 0.9:
                meta["creationTimestamp"] = stamp(t0_ns - rng.randrange(0, 10 * 86400) * 10 ** 9)
            if rng.random() < 0.04:
                meta["deletionTimestamp"] = stamp(now)
            ids = sorted(rng.sample(range(n_clusters), rng.randrange(0, max_list + 1)))
            fed = {f"c{c}": rng.randrange(1, 4) for c in ids}
            r = rng.random()
            mem = dict(fed) if r < 0.45 else dict(prev.get(k, fed)) if r < 0.7 else \
                {c: v + (rng.random() < 0.3) for c, v in fed.items()}
            prev[k] = mem
            cs = [dict(clusterName=c, status=dict(observedGeneration=v)) for c, v in fed.items()]
            r = rng.random()
            if cs and r < 0.04:
                del cs[rng.randrange(len(cs))]["clusterName"]
            elif cs and r < 0.08:
                cs[rng.randrange(len(cs))]["status"] = {}
            elif cs and r < 0.12:
                cs.append(dict(cs[0], status=dict(observedGeneration=cs[0]["status"].get("observedGeneration", 1) + 1)))
            members = [(c, dict(status=dict(observedGeneration=v))) for c, v in mem.items()]
            if members and rng.random() < 0.04:
                members[rng.randrange(len(members))] = (members[0][0], dict(status={}))
            status = None if rng.random() < 0.05 else dict(metadata={}, clusterStatus=cs)
            events.append(dict(key=k, obj=dict(metadata=meta), status_enabled=rng.random() < 0.9, status=status,
                               members=members))
        out.append((now, events))
    return out


def gen_revisions(seed: int, O: int, steady: float = 0.85, history: int = 4, env: int = 24, long_every: int = 0):
    """A synthetic revision-history batch (history.RevisionBatch): ``O`` federated Deployments whose patch is a pod
    template of ``env`` environment variables (about 60 bytes each; every ``long_every``-th object, if set, has 100
    times as many) and their listed ControllerRevisions. A share ``steady`` of the objects is in its steady state: one
    current revision that holds the patch, the highest Revision and every wanted label, and ``history`` old ones
    within a limit of ``history``, so nothing is to be done. The others are rolling: no current revision (a create),
    ``history + 2`` old ones (two deletes), a third of them with a current revision numbered too low (a renumber)
    and one old revision without the object's labels (a relabel). Old revisions hold the patch of an earlier image
    tag: the same length as the current patch, different in one byte near the end."""
    from . import gojson, history as H

    rng = np.random.default_rng([seed, 0x726576])

    def template(n_env, tag):
        return {"metadata": {"labels": {"app": "web", "tier": "frontend"}},
                "spec": {"containers": [{"name": "main", "image": f"registry.example/web:{tag}",
                                         "env": [{"name": f"SETTING_{k:04d}", "value": f"value-of-setting-{k:04d}-@@ID@@"} for k in range(n_env)],
                                         "resources": {"limits": {"cpu": "500m", "memory": "1Gi"}}}],
                         "terminationGracePeriodSeconds": 30}}

    base = {(long_, tag): gojson.revision_patch(template(env * (100 if long_ else 1), tag)) for long_ in (False, True) for tag in "0123456789"}
    batch = H.RevisionBatch()
    plans = []
    for i in range(O):
        long_ = bool(long_every) and i % long_every == long_every - 1
        ident = f"{i:06d}".encode()
        tags = rng.permutation(10)
        is_steady = rng.random() < steady
        n_old = history if is_steady else history + 2
        plans.append((i, long_, ident, tags, is_steady, n_old, int(rng.integers(0, 3))))
    # every patch and data string, then their hashes in one vector pass (the listed revisions carry true hash labels)
    strings, where = [], []
    for i, long_, ident, tags, is_steady, n_old, kind in plans:
        for t in tags[:n_old + 1]:  # [0]: the object's own patch, the others its older revisions'
            strings.append(base[(long_, str(int(t)))].replace(b"@@ID@@", ident))
    lens = np.array([len(s) for s in strings], np.int64)
    offs = np.concatenate(([0], np.cumsum(lens)[:-1])).astype(np.int64)
    blob = np.frombuffer(b"".join(strings), np.uint8)
    body = H.fnv_numpy(blob, offs, lens)
    at = 0
    for i, long_, ident, tags, is_steady, n_old, kind in plans:
        name, uid = f"web-{i:06d}", f"uid-{i:06d}"
        wanted = {"uid": uid, "app": "web", "team": f"team-{i % 7}"}

        def label_of(k):  # the hash label NewControllerRevision gave it: FNV over the data, then the collision count "0"
            h = int(body[at + k])
            h = ((h * 16777619) & 0xFFFFFFFF) ^ ord("0")
            return H.hash_label(h)

        def rev(k, number, labels=None, t=0):
            hl = label_of(k)
            lab = dict(wanted if labels is None else labels)
            lab[H.HASH_LABEL] = hl
            return {"metadata": {"name": H.revision_name(name, hl), "labels": lab, "creationTimestamp": 1700000000 + t},
                    "revision": number, "data": strings[at + k]}

        revs = [rev(k, k, t=k) for k in range(1, n_old + 1)]
        if is_steady:
            revs.append(rev(0, n_old + 1, t=n_old + 1))
        else:
            if kind == 0:
                revs.insert(1, rev(0, 1, t=n_old + 1))  # a current revision numbered too low
            revs[-1]["metadata"]["labels"] = {"uid": uid, H.HASH_LABEL: revs[-1]["metadata"]["labels"][H.HASH_LABEL]}
        batch.add(name, wanted, history, 0, strings[at], revs)
        at += n_old + 1
    return batch
