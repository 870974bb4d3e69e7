"""Case builders shared by the deletion tests: worlds in deletion_ref.py's form, their packing into the calls' arrays
(written here by hand, not through deletion.DeletionBatch, which has its own test) and the reference's answers as the
arrays the calls return."""
import functools
import itertools

import numpy as np

import deletion_ref as R

FILL = 0xA5
PAD = 67  # canary elements behind every output
OP = {None: 0, R.DELETE: 3, R.REMOVE_LABEL: 4}
STATUS = {R.OK: 0, R.ERROR: 1, R.RECHECK: 2}
REASONS = ("", "TimedOut", "RetrievalFailed", "NotReady", "OpsFailed", "Waiting", "CheckTimedOut", "CheckNotReady", "ChecksFailed")
ACT = {"delete-history": 1, "remove-finalizer": 2, "nothing": 4, "record-error": 8}
CHK = {"get_failed": 1, "deleting": 2, "labelled": 4, "unlabelled": 8}
PLAN_KEYS = ("cluster_flags", "obj_flags", "obj_ob_off", "ob_cluster", "ob_flags")
PLAN_OUT = ("out_op", "n_ops", "n_remaining", "n_retrieval_failed", "obj_pre", "obj_first")
FINISH_OUT = ("obj_status", "obj_reason", "obj_then", "n_failed_ops", "n_failed_checks")

# the five object arms and the five legal observation states
ARMS = {"nothing": {"finalizer": False, "orphan": ""}, "delete": {"finalizer": True, "orphan": ""},
        "orphan_adopted": {"finalizer": True, "orphan": "adopted"}, "orphan_all": {"finalizer": True, "orphan": "all"},
        "possible_orphan": None}
OBSERVATIONS = {"failed": "error", "exists": {"deleting": False, "adopted": False}, "deleting": {"deleting": True, "adopted": False},
                "adopted": {"deleting": False, "adopted": True}, "deleting_adopted": {"deleting": True, "adopted": True}}


def fed_of(arm, k=0):
    f = ARMS[arm]
    return None if f is None else dict(f, kind="FederatedDeployment", key=f"ns/obj-{k}")


def world(arm, members=None, op_ok=None, wait=False, check_wait=False, checks=None, k=0):
    return {"fed": fed_of(arm, k), "members": dict(members or {}), "op_ok": dict(op_ok or {}), "wait_timed_out": wait,
            "check_timed_out": check_wait, "checks": dict(checks or {})}


def cluster_names(C):
    return [f"c{i:05d}" for i in range(C)]


def clusters_of(ready):
    return list(zip(cluster_names(len(ready)), [bool(r) for r in ready]))


def obj_flags_of(fed):
    if fed is None:
        return 8
    return (1 if fed["finalizer"] else 0) | {"": 0, "all": 2, "adopted": 4}[fed["orphan"]]


def ob_flags_of(m):
    return 8 if m == "error" else 1 | (2 if m["deleting"] else 0) | (4 if m["adopted"] else 0)


def pack(worlds, clusters, clusters2=None):
    """The keyword arguments of Context.deletion_finish (PLAN_KEYS of them: Context.deletion_plan's). Cluster flags
    carry the finalizer bit beside the ready bit on even ids, so that a bit the calls must ignore is there."""
    clusters2 = clusters if clusters2 is None else clusters2
    ids = {n: i for i, (n, _) in enumerate(clusters)}
    flags = lambda cl: np.array([(1 if r else 0) | (8 if i % 2 == 0 else 0) for i, (_, r) in enumerate(cl)], np.uint8)  # noqa: E731
    ob_off, ob_cl, ob_fl, ok, k_off, k_cl, k_fl = [0], [], [], [], [0], [], []
    for w in worlds:
        for c, n in sorted((ids[n], n) for n in w["members"]):
            ob_cl.append(c)
            ob_fl.append(ob_flags_of(w["members"][n]))
            ok.append(1 if w["op_ok"].get(n, True) else 0)
        ob_off.append(len(ob_cl))
        for c, n in sorted((ids[n], n) for n in w["checks"]):
            k_cl.append(c)
            k_fl.append(CHK[w["checks"][n]])
        k_off.append(len(k_cl))
    return dict(cluster_flags=flags(clusters), obj_flags=np.array([obj_flags_of(w["fed"]) for w in worlds], np.uint8),
                obj_ob_off=np.array(ob_off, np.int32), ob_cluster=np.array(ob_cl, np.int32), ob_flags=np.array(ob_fl, np.uint8),
                op_ok=np.array(ok, np.uint8),
                obj_wait=np.array([(1 if w["wait_timed_out"] else 0) | (2 if w["check_timed_out"] else 0) for w in worlds], np.uint8),
                chk_off=np.array(k_off, np.int32), chk_cluster=np.array(k_cl, np.int32), chk_flags=np.array(k_fl, np.uint8),
                chk_cluster_flags=flags(clusters2))


def plan_args(arr):
    return {k: arr[k] for k in PLAN_KEYS}


def want_of(worlds, clusters, clusters2=None):
    """(the reference's answers as both calls' output arrays, the traces)."""
    ids = {n: i for i, (n, _) in enumerate(clusters)}
    out = {k: [] for k in PLAN_OUT + FINISH_OUT}
    traces = []
    for w in worlds:
        result, t = R.reconcile(w, clusters, clusters2)
        traces.append((result, t))
        ops = dict(t.ops)
        out["out_op"] += [OP[ops.get(n)] for _, n in sorted((ids[n], n) for n in w["members"])]
        out["n_ops"].append(len(t.ops))
        out["n_remaining"].append(len(t.remaining))
        out["n_retrieval_failed"].append(len(t.retrieval_failed))
        out["obj_pre"].append((1 if t.retrieval_failed else 0) | (2 if t.unready else 0))
        at = t.actions.index("ops") if "ops" in t.actions else len(t.actions)
        first, then = t.actions[:at], t.actions[at + 1:]
        out["obj_first"].append(sum(ACT[a] for a in first))
        out["obj_status"].append(STATUS[result])
        out["obj_reason"].append(REASONS.index(t.reason))
        out["obj_then"].append(sum(ACT[a] for a in then))
        out["n_failed_ops"].append(t.failed_ops)
        out["n_failed_checks"].append(t.failed_checks if t.checked else 0)
    dt = {"out_op": np.uint8, "obj_pre": np.uint8, "obj_first": np.uint8, "obj_status": np.uint8, "obj_reason": np.uint8, "obj_then": np.uint8}
    return {k: np.array(v, dt.get(k, np.int32)) for k, v in out.items()}, traces


def same(got, want, keys, n_pad=0, fill=FILL):
    """None, or what differs first; the ``n_pad`` elements behind every output must still hold the fill pattern."""
    for k in keys:
        g, w = np.asarray(got[k]), np.asarray(want[k])
        if len(g) != len(w) + n_pad:
            return f"{k}: length {len(g)}, expected {len(w) + n_pad}"
        if g[:len(w)].tolist() != w.tolist():
            i = int(np.flatnonzero(g[:len(w)] != w)[0])
            return f"{k}[{i}]: got {g[i]}, expected {w[i]}"
        if n_pad and not (g[len(w):].view(np.uint8) == fill).all():
            return f"{k}: written beyond its {len(w)} elements"
    return None


# ------------------------------------------------------------------ batches
@functools.lru_cache(maxsize=None)
def truth_table():
    """5 object arms x ready / unready x the 5 observation states as one batch over three clusters: the observation
    sits on c0 (ready) or on c1 (unready), c2 is ready; then the same 50 objects with a second, plain member on c2.
    → (worlds, clusters)."""
    ws = []
    for both in (False, True):
        for arm, ready, ob in itertools.product(ARMS, (True, False), OBSERVATIONS):
            members = {"c00000" if ready else "c00001": OBSERVATIONS[ob]}
            if both:
                members["c00002"] = OBSERVATIONS["exists"]
            ws.append(world(arm, members, k=len(ws)))
    return ws, clusters_of([True, False, True])


def truth_batches():
    """The truth table, and the same objects with every cluster ready (so that no object ends at NotReady)."""
    ws, clusters = truth_table()
    return [(ws, clusters), (ws, clusters_of([True, True, True]))]


def random_worlds(seed, n, C, max_members=6, unready=(), p_empty=0.2, sizes=None):
    """n seeded worlds over C clusters; ``sizes``: the number of members of each (default: random up to max_members)."""
    rng = np.random.default_rng([seed, 0xDE1])
    names = cluster_names(C)
    arms, obs, answers = list(ARMS), list(OBSERVATIONS), list(CHK)
    ws = []
    for k in range(n):
        m = int(sizes[k]) if sizes is not None else (0 if rng.random() < p_empty else int(rng.integers(1, max_members + 1)))
        picked = rng.choice(C, size=min(m, C), replace=False) if m else []
        members = {names[c]: OBSERVATIONS[obs[int(rng.choice(len(obs), p=[0.04, 0.5, 0.2, 0.2, 0.06]))]] for c in picked}
        op_ok = {n_: bool(rng.random() >= 0.05) for n_ in members}
        checks = {names[c]: answers[int(rng.integers(0, 4))] for c in rng.choice(C, size=min(int(rng.integers(0, 3)), C), replace=False)}
        ws.append(world(arms[int(rng.choice(5, p=[0.1, 0.5, 0.15, 0.15, 0.1]))], members, op_ok, rng.random() < 0.05,
                        rng.random() < 0.05, checks, k))
    ready = np.ones(C, bool)
    ready[list(unready)] = False
    return ws, clusters_of(ready)


def precedence_worlds():
    """One object per pair of adjacent reasons with both conditions true → (worlds, clusters, clusters2, the expected
    reasons). The first listing needs an unready cluster for some and none for others, so: two batches."""
    ex, failed = OBSERVATIONS["exists"], "error"
    a = [  # c2 is unready at the first listing
        (world("delete", {"c00000": ex, "c00001": failed}, wait=True), "TimedOut"),
        (world("delete", {"c00001": failed}), "RetrievalFailed"),
        (world("delete", {"c00000": ex}, op_ok={"c00000": False}), "NotReady"),
        (world("orphan_all", {"c00000": ex, "c00001": failed}, wait=True), "TimedOut"),
        (world("possible_orphan", {"c00000": ex}, op_ok={"c00000": False}), "NotReady"),
    ]
    b = [  # every cluster ready at the first listing, c2 unready at the second
        (world("delete", {"c00000": ex}, op_ok={"c00000": False}), "OpsFailed"),          # and remaining clusters
        (world("delete", {"c00000": ex}, check_wait=True, checks={"c00001": "labelled"}), "Waiting"),  # and a check time-out
        (world("delete", {}, check_wait=True), "CheckTimedOut"),                            # and an unready cluster
        (world("delete", {}, checks={"c00001": "labelled"}), "CheckNotReady"),             # and a failed check
        (world("orphan_adopted", {"c00000": OBSERVATIONS["adopted"]}, op_ok={"c00000": False}), "OpsFailed"),
        (world("possible_orphan", {"c00000": ex}, op_ok={"c00000": False}), "OpsFailed"),
    ]
    c = [  # every cluster ready at both
        (world("delete", {}, checks={"c00001": "labelled"}), "ChecksFailed"),
        (world("delete", {}, checks={"c00001": "unlabelled"}), ""),
        (world("delete", {}, wait=True), ""),  # Wait() over no operation cannot time out
    ]
    r3 = clusters_of([True, True, True])
    u3 = clusters_of([True, True, False])
    return [([w for w, _ in a], u3, u3, [r for _, r in a]), ([w for w, _ in b], r3, u3, [r for _, r in b]),
            ([w for w, _ in c], r3, r3, [r for _, r in c])]


# ------------------------------------------------------------------ objects as dicts (the packer's and the reconciler's inputs)
FINALIZER_SYNC_CONTROLLER = "kubeadmiral.io/sync-controller"
MANAGED_LABEL = "kubeadmiral.io/managed"
FIN = "kubeadmiral.io/cascading-delete-x"


def cluster_obj(name, ready=True):
    return {"metadata": {"name": name, "finalizers": [FIN]}, "status": {"conditions": [{"type": "Ready", "status": "True" if ready else "False"}]}}


def fed_obj(name, finalizer=True, orphan=None, internal=None):
    ann = {}
    if orphan is not None:
        ann["kubeadmiral.io/orphan"] = orphan
    if internal is not None:
        ann["internal.kubeadmiral.io/orphan"] = internal
    return {"kind": "FederatedDeployment", "metadata": {"name": name, "namespace": "ns", "deletionTimestamp": "2024-05-01T00:00:00Z",
                                                        "finalizers": ["other"] + ([FINALIZER_SYNC_CONTROLLER] if finalizer else []),
                                                        "annotations": ann}}


def member_obj(deleting=False, adopted=False, labelled=True):
    md = {"name": "m", "labels": {MANAGED_LABEL: "true"} if labelled else {"x": "y"}}
    if deleting:
        md["deletionTimestamp"] = "2024-05-01T00:00:00Z"
    if adopted:
        md["annotations"] = {"kubeadmiral.io/adopted": "true"}
    return {"metadata": md}


def world_of_objects(fed, members):
    """A packer object as deletion_ref.py's world, by hand."""
    if fed is None:
        f = None
    else:
        ann = fed["metadata"]["annotations"]
        orphan = ann.get("internal.kubeadmiral.io/orphan", ann.get("kubeadmiral.io/orphan", ""))
        f = {"finalizer": FINALIZER_SYNC_CONTROLLER in fed["metadata"]["finalizers"], "orphan": orphan if orphan in ("all", "adopted") else "",
             "kind": fed["kind"], "key": "ns/" + fed["metadata"]["name"]}
    ms = {}
    for n, m in members.items():
        if n == "zz" or m is None:
            continue
        ms[n] = "error" if isinstance(m, Exception) else {"deleting": "deletionTimestamp" in m["metadata"],
                                                          "adopted": (m["metadata"].get("annotations") or {}).get("kubeadmiral.io/adopted") == "true"}
    return {"fed": f, "members": ms, "op_ok": {}, "wait_timed_out": False, "check_timed_out": False, "checks": {}}


def worlds_of_arrays(arr, objects):
    """deletion_ref.py's worlds of some objects of a batch given as arrays."""
    names = cluster_names(len(arr["cluster_flags"]))
    arms = {0: "nothing", 1: "delete", 5: "orphan_adopted", 3: "orphan_all", 2: "nothing", 4: "nothing", 8: "possible_orphan"}
    answers = {v: k for k, v in CHK.items()}
    worlds = []
    for o in objects:
        lo, hi = int(arr["obj_ob_off"][o]), int(arr["obj_ob_off"][o + 1])
        members, ok = {}, {}
        for i in range(lo, hi):
            f, n = int(arr["ob_flags"][i]), names[int(arr["ob_cluster"][i])]
            members[n] = "error" if f & 8 else {"deleting": bool(f & 2), "adopted": bool(f & 4)}
            ok[n] = bool(arr["op_ok"][i])
        checks = {names[int(arr["chk_cluster"][i])]: answers[int(arr["chk_flags"][i])] for i in range(int(arr["chk_off"][o]), int(arr["chk_off"][o + 1]))}
        w = int(arr["obj_wait"][o])
        worlds.append(world(arms[int(arr["obj_flags"][o])], members, ok, bool(w & 1), bool(w & 2), checks, k=o))
    return worlds
