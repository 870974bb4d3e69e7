"""The deletion arm of the sync controller's reconcile, object by object and cluster by cluster, over dicts, lists and
sets: the yardstick of kad_deletion_plan / kad_deletion_finish and of deletion.py. Written from the reference's text
(pkg/controllers/sync/controller.go and sync/dispatch/), function by function with its line numbers, and independent of
deletion.py's array code. The reference has no Go test of these functions (no *_test.go calls ensureDeletion,
deleteFromClusters, removeManagedLabel, handleDeletionInClusters or ensureRemovedOrUnmanaged), so nothing is
transcribed under tests/golden/ for them.

The world of one object:
    fed       None (no federated object: FederatedResource returned possibleOrphan), or
              {"finalizer": bool, "orphan": "" | "all" | "adopted", "kind": str, "key": str}
    members   cluster name -> "error" (the informer lookup failed) or {"deleting": bool, "adopted": bool}; no key: the
              informer holds no object there
    op_ok     cluster name -> bool, what the operation's goroutine sent to resultChan (no key: True)
    wait_timed_out / check_timed_out   the dispatcher's Wait() ran out of time (where it had an operation to wait for)
    checks    cluster name -> "get_failed" | "deleting" | "labelled" | "unlabelled": the answer of
              CheckRemovedOrUnlabeled's GET; no key: NotFound
clusters / clusters2: [(name, ready)], GetJoinedClusters at handleDeletionInClusters and at ensureRemovedOrUnmanaged.
"""

DELETE, REMOVE_LABEL = "delete", "remove-label"
OK, ERROR, RECHECK = "OK", "Error", "Recheck"
TIMEOUT = "30s"  # operation.go:70, printed with %v


class Trace:
    """What one reconcile did, in order."""

    def __init__(self):
        self.ops = []               # (cluster, DELETE | REMOVE_LABEL) as dispatched
        self.remaining = []         # deleteFromClusters' remainingClusters
        self.retrieval_failed = []
        self.unready = []
        self.actions = []           # "delete-history", "remove-finalizer", "record-error", "nothing", with "ops" between
        self.failed_ops = 0
        self.failed_checks = 0
        self.checked = False
        self.error = None           # the error ensureDeletion / reconcile logs
        self.recorded_error = None  # fedResource.RecordError's text
        self.reason = ""


def wait(results, timed_out):
    """operationDispatcherImpl.Wait (operation.go:75-100): (ok, timeoutErr)."""
    ok = True
    if timed_out and len(results) > 0:  # the loop over operationsInitiated runs at least once
        return False, f"Failed to finish {len(results)} operations in {TIMEOUT}"
    for r in results:
        if not r:
            ok = False
    return ok, None


def handle_deletion_in_clusters(world, clusters, deletion_func, t):
    """controller.go:923-979 → (ok, err)."""
    results = []
    for name, ready in clusters:                          # :938
        if not ready:                                     # :941-944
            t.unready.append(name)
            continue
        obj = world["members"].get(name)                  # :946-952
        if obj == "error":                                # :953-958
            t.retrieval_failed.append(name)
            continue
        if obj is None:                                   # :959-961
            continue
        op = deletion_func(name, obj)                     # :963
        if op is not None:
            t.ops.append((name, op))
            results.append(world["op_ok"].get(name, True))
    t.failed_ops = sum(1 for r in results if not r)
    ok, timeout_err = wait(results, world.get("wait_timed_out", False))  # :965
    if timeout_err is not None:                           # :966-968
        t.reason = "TimedOut"
        return False, timeout_err
    if t.retrieval_failed:                                # :969-974
        t.reason = "RetrievalFailed"
        return False, "failed to retrieve a managed resource for the following cluster(s): " + ", ".join(t.retrieval_failed)
    if t.unready:                                         # :975-977
        t.reason = "NotReady"
        return False, "the following clusters were not ready: " + ", ".join(t.unready)
    return ok, None                                       # :978


def remove_managed_label(world, clusters, t):
    """controller.go:793-817 → err."""
    def f(name, obj):                                     # :802-808
        if obj["deleting"]:
            return None
        return REMOVE_LABEL
    ok, err = handle_deletion_in_clusters(world, clusters, f, t)
    if err is not None:                                   # :810-812
        return err
    if not ok:                                            # :813-815
        t.reason = "OpsFailed"
        return "failed to remove the label from resources in one or more clusters."
    return None


def delete_from_cluster(fed, obj):
    """controller.go:819-844 with respectOrphaningBehavior (deleteFromClusters passes true, :858). The dispatcher's
    Delete still runs for an object that is being deleted: it strips the retain finalizer and returns before the
    DELETE (dispatch/unmanaged.go:93-140), so it is an operation like any other."""
    should_be_orphaned = fed["orphan"] == "all" or (fed["orphan"] == "adopted" and obj["adopted"])  # :834-836
    return REMOVE_LABEL if should_be_orphaned else DELETE  # :837-843


def ensure_removed_or_unmanaged(world, clusters2, t):
    """controller.go:889-919 → err."""
    t.checked = True
    unready, results = [], []
    for name, ready in clusters2:                         # :901
        if not ready:                                     # :902-905
            unready.append(name)
            continue
        answer = world["checks"].get(name)                # CheckRemovedOrUnlabeled, dispatch/checkunmanaged.go:71-100
        if answer is None:                                # NotFound :83-85
            results.append(True)
        elif answer == "get_failed":                      # :86-89
            results.append(False)
        elif answer == "deleting":                        # :90-93
            results.append(False)
        elif answer == "unlabelled":                      # :94-96
            results.append(True)
        else:                                             # :97-98
            results.append(False)
    t.failed_checks = sum(1 for r in results if not r)
    ok, timeout_err = wait(results, world.get("check_timed_out", False))  # :908
    if timeout_err is not None:                           # :909-911
        t.reason = "CheckTimedOut"
        return timeout_err
    if unready:                                           # :912-914
        t.reason = "CheckNotReady"
        return "the following clusters were not ready: " + ", ".join(unready)
    if not ok:                                            # :915-917
        t.reason = "ChecksFailed"
        return "one or more checks failed"
    return None


def delete_from_clusters(world, clusters, clusters2, t):
    """controller.go:846-882 → (recheckRequired, err)."""
    fed = world["fed"]

    def f(name, obj):                                     # :856-859
        t.remaining.append(name)
        return delete_from_cluster(fed, obj)
    ok, err = handle_deletion_in_clusters(world, clusters, f, t)
    if err is not None:                                   # :861-863
        return False, err
    if not ok:                                            # :864-866
        t.reason = "OpsFailed"
        return False, "failed to remove managed resources from one or more clusters."
    if len(t.remaining) > 0:                              # :867-871
        t.reason = "Waiting"
        return True, None
    err = ensure_removed_or_unmanaged(world, clusters2, t)  # :872
    if err is not None:                                   # :873-875
        return False, "failed to verify that managed resources no longer exist in any cluster: " + err
    t.actions.append("delete-history")                    # :877-879
    return False, None


def ensure_deletion(world, clusters, clusters2, t):
    """controller.go:723-789 → worker result."""
    fed = world["fed"]
    if not fed["finalizer"]:                              # :734-739
        t.actions.append("nothing")
        return OK
    if fed["orphan"] == "all":                            # :741-767
        t.actions.append("delete-history")                # :744
        t.actions.append("remove-finalizer")              # :749
        t.actions.append("ops")
        err = remove_managed_label(world, clusters, t)    # :760
        if err is not None:                               # :761-765
            t.error = err
            return ERROR
        return OK
    t.actions.append("ops")
    recheck, err = delete_from_clusters(world, clusters, clusters2, t)  # :770
    if err is not None:                                   # :771-776
        t.error = err
        t.recorded_error = 'failed to delete %s "%s": %s' % (fed["kind"], fed["key"], err)
        t.actions.append("record-error")
        return ERROR
    if recheck:                                           # :777-779
        return RECHECK
    t.actions.append("remove-finalizer")                  # :780
    return OK


def reconcile(world, clusters, clusters2=None):
    """controller.go:340-378 → (worker result, Trace)."""
    t = Trace()
    clusters2 = clusters if clusters2 is None else clusters2
    if world["fed"] is None:                              # possibleOrphan :350-363
        t.actions.append("ops")
        err = remove_managed_label(world, clusters, t)
        if err is not None:
            t.error = err
            return ERROR, t
        return OK, t
    return ensure_deletion(world, clusters, clusters2, t), t  # :376-378


def decide(world_fed, ready, observation):
    """One (object, observed cluster) pair through reconcile: (op or None, counted as remaining, counted as a retrieval
    failure). observation: "error" or {"deleting", "adopted"}."""
    world = {"fed": world_fed, "members": {"c": observation}, "op_ok": {}, "checks": {}}
    _, t = reconcile(world, [("c", ready)])
    return (t.ops[0][1] if t.ops else None), bool(t.remaining), bool(t.retrieval_failed)
