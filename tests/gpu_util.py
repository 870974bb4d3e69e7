"""Helpers shared by the GPU parity tests, and the inputs of the boundary tests (test_gpu_boundaries.py runs
them on the GPU, test_boundary_inputs.py checks on the C oracle alone that they reach the edges)."""
import functools
import os

import numpy as np

from kubeadmiral_amd import framework as F
from kubeadmiral_amd import pack, synth
from kubeadmiral_amd import types as T
from oracle import ref


def c_oracle(snap, batch, fwk):
    return ref.schedule(snap, batch, fwk, n_threads=min(16, os.cpu_count() or 1))


def assert_same(got, want, what=""):
    eq = got.equal_rows(want) & (got.flags == want.flags)
    bad = np.nonzero(~eq)[0]
    if len(bad):
        w = int(bad[0])
        raise AssertionError(f"{what}: {len(bad)} rows differ; first w={w}: gpu={got.row(w)} flags={got.flags[w]} "
                             f"oracle={want.row(w)} flags={want.flags[w]}")


# ------------------------------------------------------------------ boundary inputs
# Cluster counts at which the route (kad_route.h) changes kernels (nch = ceil(C / 64)): exact chunk
# multiples (no tail chunk) and one past them (one live lane in the last chunk).
SWEEP_CS = [64, 128, 192, 256, 257, 320, 449, 512, 513, 961, 1024, 1025, 4096, 4097, 8192, 8193, 12288, 16384, 16385]
SWEEP_W = 64
# the sweep's third profile rotates over the fuzz profiles that filter on more than placement or resources
# (FUZZ_PROFILES 2: affinity + taints, 3: Fit + APIResources + placement with Most / Balanced scores), so that
# some units end without a feasible cluster at every C
SWEEP_ROTATION = (2, 3)
SWEEP_PROFILES = ("default", "none", "rotating")
MAX_C = 65535  # the ABI's maximum (check_snapshot_header) and the largest u16 cluster id
LIST_NS = (0, 1, 63, 64, 65, 255, 256, 257, 511, 512, 513)
LIST_CS = (1000, 1100)  # wide kernel (16 chunks) / schedule_lean_kernel<0> (18 chunks)
# chosen so that MaxCluster cuts a run of tied totals on each side of both cuts (test_boundary_inputs.py)
LIST_SEEDS = {1000: 11, 1100: 2}
SMALL_WS = (1, 3, 4, 5, 15, 16, 17, 65)


def nch_of(C):
    return (C + 63) // 64


def default_framework():
    return F.Framework(F.default_enabled_plugins())


def sweep_framework(C, which):
    if which == "default":
        return default_framework()
    if which == "none":
        return synth.fuzz_framework(0)
    return synth.fuzz_framework(SWEEP_ROTATION[SWEEP_CS.index(C) % len(SWEEP_ROTATION)])


def serve_deployments(clusters):
    """Every cluster serves apps/v1 Deployment (in place): the probe units' GVK."""
    for c in clusters:
        if not any((a.group, a.version, a.kind) == synth.GVKS[0] for a in c.api_resource_types or []):
            c.api_resource_types = list(c.api_resource_types or []) + [T.APIResource(*synth.GVKS[0])]


def plain_unit(name, place=None, max_clusters=None):
    """A Duplicate unit no plugin but PlacementFilter can reject: tolerates every taint, no selector or
    affinity, request 0, a GVK every cluster serves (after serve_deployments)."""
    return T.SchedulingUnit(group="apps", version="v1", kind="Deployment", resource="deployments",
                            namespace="default", name=name, desired_replicas=3,
                            scheduling_mode=T.SCHEDULING_MODE_DUPLICATE,
                            tolerations=[T.Toleration(operator=T.TOLERATION_OP_EXISTS)],
                            cluster_names=None if place is None else set(place), max_clusters=max_clusters)


def probe_units(clusters):
    """Four units that put a result on the edges of the cluster range: placement {C-1} (the last live lane),
    {64 * (nch - 1)} (the first lane of the last chunk), {0}, and one every cluster is feasible for with no
    MaxClusters (count == C under every profile)."""
    C = len(clusters)
    names = [c.name for c in clusters]
    return [plain_unit("probe-last", [names[C - 1]]), plain_unit("probe-chunk", [names[64 * (nch_of(C) - 1)]]),
            plain_unit("probe-first", [names[0]]), plain_unit("probe-all")]


# seed per sweep C: chosen so that under the default and the rotating profile at least 10 units end ST_OK
# with a cluster and at least 5 end without a feasible one (test_boundary_inputs.py asserts it)
SWEEP_SEEDS = {C: 8100 + i for i, C in enumerate(SWEEP_CS)}
MAX_C_SEED = 8190


@functools.lru_cache(maxsize=None)
def fuzz_with_probes(seed, C, W):
    """(clusters, units, snapshot): gen_fuzz(seed, W, C) with Deployments served everywhere, plus probe_units."""
    clusters, units = synth.gen_fuzz(seed, W=W, C=C)
    serve_deployments(clusters)
    return clusters, units + probe_units(clusters), pack.Snapshot(clusters)


@functools.lru_cache(maxsize=None)
def sweep_case(C, which):
    """(snapshot, batch, framework, oracle result) of the C sweep under profile ``which``."""
    _, units, snap = fuzz_with_probes(SWEEP_SEEDS[C], C, SWEEP_W)
    fwk = sweep_framework(C, which)
    batch = pack.Batch(snap, fwk, units)
    return snap, batch, fwk, c_oracle(snap, batch, fwk)


@functools.lru_cache(maxsize=None)
def max_c_case():
    """C = 65535, 8 fuzz units and the probes, under the default profile."""
    _, units, snap = fuzz_with_probes(MAX_C_SEED, MAX_C, 8)
    fwk = default_framework()
    batch = pack.Batch(snap, fwk, units)
    return snap, batch, fwk, c_oracle(snap, batch, fwk)


@functools.lru_cache(maxsize=None)
def zero_c_case():
    """C = 0: four Duplicate units (plain, with a placement, with MaxClusters, with a request) against an
    empty snapshot, under the default profile."""
    units = [plain_unit("zero-0"), plain_unit("zero-1", ["ghost-cluster"]), plain_unit("zero-2", None, 1),
             plain_unit("zero-3")]
    units[3].resource_request = T.Resource(250, 1 << 30)
    snap = pack.Snapshot([])
    fwk = default_framework()
    batch = pack.Batch(snap, fwk, units)
    return snap, batch, fwk, c_oracle(snap, batch, fwk)


def list_ns(C):
    return LIST_NS + (C - 1, C)


@functools.lru_cache(maxsize=None)
def list_case(C):
    """Exact feasible-list lengths on C clean clusters (gen_clusters, half of them quantised to one resource
    shape as gen_fuzz does, so totals tie): for each n of list_ns(C) three plain units whose placement is
    exactly the first n, the last n and n strided cluster names, so n is the feasible-list length; MaxClusters
    cycles over None, 1 and n - 1 (n = 0: placement on a name no cluster has). Returns (snapshot, batch, framework, oracle result, [(n, max_clusters)])."""
    rng = np.random.default_rng(LIST_SEEDS[C])
    clusters = synth.gen_clusters(rng, C)
    for c in clusters:
        if rng.random() < 0.5:
            c.allocatable["cpu"], c.available["cpu"] = "8", "4"
            c.allocatable["memory"], c.available["memory"] = "16Gi", "8Gi"
    names = [c.name for c in clusters]
    units, meta = [], []
    for i, n in enumerate(list_ns(C)):
        strided = [names[(j * C) // n] for j in range(n)]
        for j, place in enumerate((names[:n], names[C - n:], strided)):
            assert len(set(place)) == n
            if n == 0:  # an empty ClusterNames set filters nothing: a name no cluster has leaves none feasible
                place = ["ghost-cluster"]
            maxc = (None, 1, n - 1)[(i + j) % 3]
            units.append(plain_unit(f"list-{n}-{j}", place, maxc))
            meta.append((n, maxc))
    snap = pack.Snapshot(clusters)
    fwk = default_framework()
    batch = pack.Batch(snap, fwk, units)
    return snap, batch, fwk, c_oracle(snap, batch, fwk), meta


def extreme_batch(seed, C=200, W=120):
    """Fuzz batch pushed to the edges of the lean kernel's fast paths: capacities
    above 2^46 (Least/MostAllocated's exact int64 path), zero and negative
    quantities, and preferred-affinity weights of +-2^31 so totals span more
    than 2^32 (64-bit bisection; wide-key straddles go to the full kernel)."""
    rng = np.random.default_rng(seed)
    clusters, units = synth.gen_fuzz(seed, W=W, C=C)
    for c in clusters:
        r = rng.random()
        if r < 0.25:
            c.allocatable["memory"] = str(int(rng.integers(1 << 46, 1 << 52)))
            c.available["memory"] = str(int(rng.integers(0, 1 << 46)))
        elif r < 0.35:
            c.allocatable["cpu"] = "0"
            c.available["cpu"] = "0"
        elif r < 0.45:
            c.allocatable["cpu"] = f"{int(rng.integers(1, 1 << 40))}m"
            c.available["cpu"] = "1m"
    for su in units:
        ca = su.affinity.cluster_affinity if su.affinity is not None else None
        if ca is not None and ca.preferred:
            for p in ca.preferred:
                if rng.random() < 0.5:
                    p.weight = int(rng.choice([-(1 << 31), (1 << 31) - 1, -123456789, 987654321]))
    return clusters, units
