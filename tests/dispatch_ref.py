"""The checker of kad_dispatch_plan: syncToClusters cluster by cluster, as the reference walks it
(pkg/controllers/sync/controller.go:425-544), over Python sets and dicts. No bitmaps, no numpy, nothing from
kubeadmiral_amd.dispatch: the arrays are only unpacked into names and objects here, and the answer is laid out the
way the entry point lays it out.
"""

# the constants of include/kad_sched.h, restated
READY, TERMINATING, CASCADING, FINALIZER = 1, 2, 4, 8
ERROR, ORPHAN_ALL, ORPHAN_ADOPTED = 1, 2, 4
EXISTS, DELETING, ADOPTED, RETRIEVAL_FAILED = 1, 2, 4, 8
NONE, CREATE, UPDATE, DELETE, REMOVE_LABEL = range(5)
STATUSES = ("", "ClusterNotReady", "CachedRetrievalFailed", "WaitingForRemoval", "LabelRemovalTimedOut",
            "DeletionTimedOut", "ClusterTerminating", "FinalizerCheckFailed", "CreationTimedOut", "UpdateTimedOut")
ST = {s: i for i, s in enumerate(STATUSES)}
RECHECK, PLACEMENT_FAILED = 1, 2


def compute_placement(placement_names, joined, namespaced_rule, namespace_names):
    """federatedResource.ComputePlacement (resource.go:170-175) → computeNamespacedPlacement / computePlacement
    (placement.go:45-88). ``namespaced_rule``: "none" = a cluster-scoped type, or limited scope without a federated
    namespace (:55-60); "unfederated" = a namespaced type without one (:62-63); "intersect" = with one."""
    selected = set()
    for name in placement_names:               # selectedClusterNames (:101-105)
        selected.add(name)
    resource = set(joined) & selected          # computePlacement (:86-87)
    if namespaced_rule == "none":
        return resource
    if namespaced_rule == "unfederated":
        return set()
    return resource & (set(joined) & set(namespace_names))  # :66-73


def sync_to_clusters(clusters, selected, lookup, orphaning):
    """The loop of :458-544. ``clusters``: [(name, flags)] in the informer's order; ``lookup``: name → the member
    object's flags, None, or "error"; ``orphaning``: "all", "adopted" or "". Returns ([(name, op, status)], the
    operations started, shouldRecheckAfterDispatch)."""
    recorded, n_ops, recheck = [], 0, False
    for name, cf in clusters:
        is_selected = name in selected                                       # :460
        cascading_triggered = bool(cf & TERMINATING) and bool(cf & CASCADING)  # :461
        should_be_deleted = not is_selected or cascading_triggered           # :462
        if not cf & READY:                                                   # :464
            if not should_be_deleted:
                recorded.append((name, NONE, "ClusterNotReady"))             # :469
            continue
        obj = lookup.get(name)                                               # :474
        if obj == "error":
            recorded.append((name, NONE, "CachedRetrievalFailed"))           # :483
            continue
        if should_be_deleted:                                                # :488
            if obj is None:
                continue                                                     # :491
            if obj & DELETING:
                recorded.append((name, NONE, "WaitingForRemoval"))           # :495
                continue
            if cf & TERMINATING and not cf & CASCADING:
                continue                                                     # :505
            # deleteFromCluster (:819-844), respectOrphaningBehavior = cascading_triggered
            if cascading_triggered and (orphaning == "all" or (orphaning == "adopted" and obj & ADOPTED)):
                recorded.append((name, REMOVE_LABEL, "LabelRemovalTimedOut"))  # managed.go:566-570
            else:
                recorded.append((name, DELETE, "DeletionTimedOut"))          # managed.go:477-481
            n_ops += 1
            continue
        if cf & TERMINATING:                                                 # :514
            recorded.append((name, NONE, "ClusterTerminating"))
            continue
        if not cf & FINALIZER:                                               # :529
            recheck = True
            recorded.append((name, NONE, "FinalizerCheckFailed"))
            continue
        if obj is None:
            recorded.append((name, CREATE, "CreationTimedOut"))              # :540, managed.go:330
        else:
            recorded.append((name, UPDATE, "UpdateTimedOut"))                # :542, managed.go:403
        n_ops += 1
    return recorded, n_ops, recheck


def run(cluster_flags, obj_flags, obj_ns, obj_pl_off, pl_cluster, ns_pl_off, ns_cluster, obj_ob_off, ob_cluster,
        ob_flags, out_off, fill=0):
    """The arrays of one call → the outputs of kad_dispatch_plan as lists (entries at out_off[o] on, ``fill``
    behind them)."""
    name = lambda c: f"c{int(c)}" if int(c) >= 0 else f"stranger{int(c)}"  # noqa: E731
    clusters = [(name(c), int(f)) for c, f in enumerate(cluster_flags)]
    joined = [n for n, _ in clusters]
    ident = {n: c for c, n in enumerate(joined)}
    n_obj, cap = len(obj_flags), int(out_off[-1])
    out = {"out_cluster": [fill * 0x01010101 if fill < 128 else fill * 0x01010101 - 2 ** 32] * cap, "out_op": [fill] * cap,
           "out_status": [fill] * cap, "count": [0] * n_obj, "n_ops": [0] * n_obj, "n_selected": [0] * n_obj,
           "obj_result": [0] * n_obj}
    for o in range(n_obj):
        of = int(obj_flags[o])
        if of & ERROR:                                                       # :437-444
            out["obj_result"][o] = PLACEMENT_FAILED
            continue
        ns = int(obj_ns[o])
        rule = "intersect" if ns >= 0 else "none" if ns == -1 else "unfederated"
        ns_names = [name(c) for c in ns_cluster[int(ns_pl_off[ns]):int(ns_pl_off[ns + 1])]] if ns >= 0 else []
        selected = compute_placement([name(c) for c in pl_cluster[int(obj_pl_off[o]):int(obj_pl_off[o + 1])]], joined, rule, ns_names)
        lookup = {}
        for k in range(int(obj_ob_off[o]), int(obj_ob_off[o + 1])):
            f = int(ob_flags[k])
            lookup[name(ob_cluster[k])] = "error" if f & RETRIEVAL_FAILED else f
        orphaning = "all" if of & ORPHAN_ALL else "adopted" if of & ORPHAN_ADOPTED else ""
        recorded, n_ops, recheck = sync_to_clusters(clusters, selected, lookup, orphaning)
        at = int(out_off[o])
        assert len(recorded) <= int(out_off[o + 1]) - at
        for i, (n, op, status) in enumerate(recorded):
            out["out_cluster"][at + i], out["out_op"][at + i], out["out_status"][at + i] = ident[n], op, ST[status]
        out["count"][o], out["n_ops"][o], out["n_selected"][o] = len(recorded), n_ops, len(selected)
        out["obj_result"][o] = RECHECK if recheck else 0
    return out
