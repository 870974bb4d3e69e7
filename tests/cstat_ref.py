"""An independent checker for the cluster-status feature: aggregateResources
(pkg/controllers/federatedcluster/util.go:113-214) object by object over Fractions, with its own quantity reader.
Shares no code with kubeadmiral_amd/clusterstatus.py. Two forms: over node / pod dicts (:func:`aggregate`) and over
the arrays of kad_cluster_resources (:func:`run`), one entry at a time."""
import re
from fractions import Fraction

_SUF = {"": 1, "n": Fraction(1, 10**9), "u": Fraction(1, 10**6), "m": Fraction(1, 1000), "k": 10**3, "M": 10**6,
        "G": 10**9, "T": 10**12, "P": 10**15, "E": 10**18, "Ki": 2**10, "Mi": 2**20, "Gi": 2**30, "Ti": 2**40,
        "Pi": 2**50, "Ei": 2**60}
_Q = re.compile(r"^([+-]?)(\d*)(?:\.(\d*))?([A-Za-z]*|[eE][+-]?\d+)$")


def qty(s) -> Fraction:
    """A quantity string's exact value (nano precision is enough for every test input)."""
    m = _Q.match(str(s))
    assert m and (m.group(2) or m.group(3)), s
    digits = Fraction(int((m.group(2) or "0") + (m.group(3) or "")), 10 ** len(m.group(3) or ""))
    suf = m.group(4)
    mult = Fraction(10) ** int(suf[1:]) if suf[:1] in ("e", "E") and suf not in _SUF else Fraction(_SUF[suf])
    return (-digits if m.group(1) == "-" else digits) * mult


def node_ok(node) -> bool:
    spec = node.get("spec") or {}
    if spec.get("unschedulable"):
        return False
    if any(t.get("effect") in ("NoSchedule", "NoExecute") for t in spec.get("taints") or []):
        return False
    for c in (node.get("status") or {}).get("conditions") or []:
        if c.get("type") == "Ready" and c.get("status") != "True":
            return False
    return True


def pod_requests(pod) -> dict:
    spec = pod.get("spec") or {}
    total = {}
    for c in spec.get("containers") or []:
        for n, q in ((c.get("resources") or {}).get("requests") or {}).items():
            total[n] = total.get(n, Fraction(0)) + qty(q)
    for c in spec.get("initContainers") or []:
        for n, q in ((c.get("resources") or {}).get("requests") or {}).items():
            if n not in total or qty(q) > total[n]:
                total[n] = qty(q)
    for n, q in (spec.get("overhead") or {}).items():
        total[n] = total.get(n, Fraction(0)) + qty(q)
    return total


def aggregate(nodes, pods):
    """(schedulableNodes, allocatable, available) with Fraction values."""
    alloc, count = {}, 0
    for node in nodes:
        if not node_ok(node):
            continue
        count += 1
        for n, q in ((node.get("status") or {}).get("allocatable") or {}).items():
            alloc[n] = alloc.get(n, Fraction(0)) + qty(q)
    alloc.pop("pods", None)
    avail = dict(alloc)
    for pod in pods:
        if (pod.get("status") or {}).get("phase") in ("Succeeded", "Failed"):
            continue
        for n, q in pod_requests(pod).items():
            if n in avail:
                avail[n] = avail[n] - q
    return count, alloc, avail


def text(q: Fraction) -> str:
    """A quantity string of the value (plain decimal with up to nine fractional digits)."""
    n = q * 10**9
    assert n.denominator == 1
    sign, n = ("-" if n < 0 else ""), abs(int(n))
    whole, frac = divmod(n, 10**9)
    return f"{sign}{whole}" + (f".{frac:09d}".rstrip("0") if frac else "")


def run(n_res, cl_node_off, node_flags, node_ent_off, nent_res, nent_val, cl_pod_off, pod_flags, pod_ent_off, pent_res,
        pent_kind, pent_val) -> dict:
    """kad_cluster_resources' outputs as lists of Python ints, entry by entry."""
    R, K = int(n_res), len(cl_node_off) - 1
    alloc, avail, has, sched = [0] * (K * R), [0] * (K * R), [0] * K, [0] * K
    for k in range(K):
        for n in range(int(cl_node_off[k]), int(cl_node_off[k + 1])):
            if not int(node_flags[n]) & 1:
                continue
            sched[k] += 1
            for e in range(int(node_ent_off[n]), int(node_ent_off[n + 1])):
                has[k] |= 1 << int(nent_res[e])
                alloc[k * R + int(nent_res[e])] += int(nent_val[e])
        avail[k * R:(k + 1) * R] = alloc[k * R:(k + 1) * R]
        for p in range(int(cl_pod_off[k]), int(cl_pod_off[k + 1])):
            if int(pod_flags[p]) & 1:
                continue
            cont, init, over = {}, {}, {}
            for e in range(int(pod_ent_off[p]), int(pod_ent_off[p + 1])):
                r, v = int(pent_res[e]), int(pent_val[e])
                if pent_kind[e] == 0:
                    cont[r] = cont.get(r, 0) + v
                elif pent_kind[e] == 1:
                    init[r] = max(init.get(r, 0), v)
                else:
                    over[r] = over.get(r, 0) + v
            for r in set(cont) | set(init) | set(over):
                if has[k] >> r & 1:
                    avail[k * R + r] -= max(cont.get(r, 0), init.get(r, 0)) + over.get(r, 0)
    return {"alloc": alloc, "avail": avail, "has": has, "sched_nodes": sched}
