"""Call arrays for kad_cluster_resources from node and pod lists (test_cstat_host.py, test_gpu_cstat.py).

A node is (flags, [(res, value), ...]), a pod (flags, [(res, kind, value), ...]); the builder sorts a pod's entries
by (res, kind) as the ABI asks. Seeded generators give clusters of exact node, pod and entry counts."""
import numpy as np

SCHED, TERMINAL = 1, 1
POD_CHUNK = 4096  # CS_POD_CHUNK: pods per block of the long path's pod pass
BOUND = 1 << 62


class Builder:
    def __init__(self, n_res):
        self.R = n_res
        self.cn, self.nf, self.ne, self.nr, self.nv = [0], [], [0], [], []
        self.cp, self.pf, self.pe, self.pr, self.pk, self.pv = [0], [], [0], [], [], []

    def add(self, nodes, pods):
        for flags, ents in nodes:
            self.nf.append(flags)
            for r, v in ents:
                self.nr.append(r)
                self.nv.append(v)
            self.ne.append(len(self.nr))
        self.cn.append(len(self.nf))
        for flags, ents in pods:
            self.pf.append(flags)
            for r, k, v in sorted(ents, key=lambda e: (e[0], e[1])):
                self.pr.append(r)
                self.pk.append(k)
                self.pv.append(v)
            self.pe.append(len(self.pr))
        self.cp.append(len(self.pf))
        return len(self.cn) - 2

    def arrays(self):
        return dict(n_res=self.R, cl_node_off=np.array(self.cn, np.int64), node_flags=np.array(self.nf, np.uint8),
                    node_ent_off=np.array(self.ne, np.int64), nent_res=np.array(self.nr, np.uint8),
                    nent_val=np.array(self.nv, np.int64), cl_pod_off=np.array(self.cp, np.int64),
                    pod_flags=np.array(self.pf, np.uint8), pod_ent_off=np.array(self.pe, np.int64),
                    pent_res=np.array(self.pr, np.uint8), pent_kind=np.array(self.pk, np.uint8),
                    pent_val=np.array(self.pv, np.int64))


def entries_of(a, k):
    """Node + pod entries of cluster k: what the route compares with long_min."""
    n0, n1 = a["cl_node_off"][k], a["cl_node_off"][k + 1]
    p0, p1 = a["cl_pod_off"][k], a["cl_pod_off"][k + 1]
    return int(a["node_ent_off"][n1] - a["node_ent_off"][n0] + a["pod_ent_off"][p1] - a["pod_ent_off"][p0])


def route_counts(a, long_min):
    """(n_clusters, n_long, short_nodes, short_pods, n_chunks): kad_cstat_route_eval's arguments for the arrays."""
    K = len(a["cl_node_off"]) - 1
    n_long = short_nodes = short_pods = n_chunks = 0
    for k in range(K):
        nodes = int(a["cl_node_off"][k + 1] - a["cl_node_off"][k])
        pods = int(a["cl_pod_off"][k + 1] - a["cl_pod_off"][k])
        if entries_of(a, k) > long_min:
            n_long += 1
            n_chunks += -(-pods // POD_CHUNK)
        else:
            short_nodes += nodes
            short_pods += pods
    return K, n_long, short_nodes, short_pods, n_chunks


def rand_nodes(rng, R, n, p_sched=0.85, max_names=4):
    out = []
    for _ in range(n):
        m = int(rng.integers(0, min(R, max_names) + 1))
        res = sorted(int(r) for r in rng.choice(R, m, replace=False))
        out.append((SCHED if rng.random() < p_sched else 0, [(r, int(rng.integers(0, 1 << 24))) for r in res]))
    return out


def rand_pods(rng, R, n, p_term=0.15, max_ents=6):
    """Pods of 0..max_ents entries over random (res, kind) pairs, repeats of one pair included."""
    out = []
    for _ in range(n):
        m = int(rng.integers(0, max_ents + 1))
        ents = [(int(rng.integers(0, R)), int(rng.integers(0, 3)), int(rng.integers(0, 1 << 16))) for _ in range(m)]
        out.append((TERMINAL if rng.random() < p_term else 0, ents))
    return out


def exact_entries(rng, R, total):
    """A cluster of exactly ``total`` entries: three nodes naming min(R, 2) resources, pods of three entries, and a
    last pod with the rest."""
    per = min(R, 2)
    nodes = [(SCHED, [(r, int(rng.integers(1 << 30, 1 << 34))) for r in range(per)]) for _ in range(3)]
    left = total - 3 * per
    assert left >= 0
    pods = []
    while left > 0:
        m = min(3, left)
        pods.append((0, [(int(rng.integers(0, per)), int(rng.integers(0, 3)), int(rng.integers(0, 1 << 16)))
                         for _ in range(m)]))
        left -= m
    return nodes, pods


def full_run_pod(R, kind=0):
    """A pod whose entries are one run of R names."""
    return (0, [(r, kind, r + 1) for r in range(R)])


NODE_COUNTS = (0, 1, 63, 64, 65, 3 * 256 + 5)


def shapes_case(long_min, R=5, seed=1):
    """One batch: clusters of NODE_COUNTS nodes; clusters of long_min - 1, long_min and long_min + 1 entries; a
    long cluster whose pods fill two chunks and one pod of a third; pods without entries and pods naming all R
    names; a cluster without schedulable nodes, one with every pod terminal, one whose Available goes negative,
    one with nodes and no pods, one with pods and no nodes. Returns (arrays, {name: cluster index})."""
    rng = np.random.default_rng([seed, R])
    b, marks = Builder(R), {}
    for n in NODE_COUNTS:
        marks[f"nodes-{n}"] = b.add(rand_nodes(rng, R, n), rand_pods(rng, R, 2 * n + 3) + [(0, []), full_run_pod(R)])
    for d in (-1, 0, 1):
        marks[f"entries-{d}"] = b.add(*exact_entries(rng, R, long_min + d))
    marks["chunks"] = b.add(rand_nodes(rng, R, 40), [(0, [(0, 0, 3)])] * (2 * POD_CHUNK) + [(0, [(0, 0, 5), (1, 2, 7)])])
    marks["unschedulable"] = b.add([(0, [(0, 10), (1, 20)])] * 3, [(0, [(0, 0, 1)])])
    marks["terminal"] = b.add([(SCHED, [(0, 10), (1, 20)])], [(TERMINAL, [(0, 0, 1), (1, 0, 2)])] * 5)
    marks["negative"] = b.add([(SCHED, [(0, 10), (1, 0)])], [(0, [(0, 0, 8), (0, 1, 12), (0, 2, 1), (1, 0, 4)])] * 2)
    marks["no-pods"] = b.add(rand_nodes(rng, R, 9), [])
    marks["no-nodes"] = b.add([], rand_pods(rng, R, 9))
    return b.arrays(), marks


def mixed_case(K, R, seed, long_every=16, long_ents=96):
    """K small clusters, every ``long_every``-th one of about ``long_ents`` entries (long under a forced long_min
    below that), the others of at most 40."""
    rng = np.random.default_rng([seed, K, R])
    b = Builder(R)
    for k in range(K):
        if k % long_every == long_every - 1:
            b.add(rand_nodes(rng, R, 12), rand_pods(rng, R, long_ents // 2, max_ents=4) + [full_run_pod(R, 2)])
        else:
            b.add(rand_nodes(rng, R, int(rng.integers(0, 5))), rand_pods(rng, R, int(rng.integers(0, 9)), max_ents=4))
    return b.arrays()


def width_case(width, R=3, seed=5, K=70):
    """Short clusters whose mean nodes and pods per cluster make the route pick ``width`` for both passes
    (mean / 8 rounded up to a power of two): means of 8 * width - 3."""
    rng = np.random.default_rng([seed, width])
    n = 8 * width - 3
    b = Builder(R)
    for k in range(K):
        d = int(rng.integers(-2, 3)) if k < K - 1 else 0
        b.add(rand_nodes(rng, R, n + d, max_names=2), rand_pods(rng, R, n - d, max_ents=2))
    return b.arrays()


def bound_case():
    """R = 64, max value x max entries of one cluster exactly 2^62 on both sides. Cluster 0: four node entries of
    2^60 on name 0 alone (Allocatable 2^62, presence bit 0 alone), four pod entries of 2^60 (Available 0). Cluster
    1: name 63 present at 0, requests of 2^62 against it (Available -2^62). Cluster 2: presence bit 63 alone, a
    pod naming 0 and 63."""
    b = Builder(64)
    v = BOUND // 4
    b.add([(SCHED, [(0, v)])] * 4, [(0, [(0, 0, v), (0, 0, v)]), (0, [(0, 1, v), (0, 2, v)])])
    b.add([(SCHED, [(63, 0), (5, 1)])], [(0, [(63, 0, v), (63, 0, v), (63, 2, v), (63, 2, v)])])
    b.add([(SCHED, [(63, 9)])], [(0, [(0, 0, 4), (63, 0, 2), (63, 1, 3)])])
    return b.arrays()
