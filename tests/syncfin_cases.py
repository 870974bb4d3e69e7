"""Inputs for the sync-completion tests: named objects for every corner of kad_sync_finish, a seeded generator that
returns objects as dicts (syncfin_ref.finish's argument), batches of update rows for kad_sync_needs_update, and the
packing of both through kubeadmiral_amd.syncfin."""
import json
import os
import random

import syncfin_ref as R

STATUSES = ("OK", "WaitingForRemoval", "ClusterNotReady", "ClusterTerminating", "CachedRetrievalFailed",
            "ComputeResourceFailed", "ApplyOverridesFailed", "CreationFailed", "UpdateFailed", "DeletionFailed",
            "LabelRemovalFailed", "RetrievalFailed", "AlreadyExists", "FieldRetentionFailed", "SetLastReplicasetNameFailed",
            "VersionRetrievalFailed", "ClientRetrievalFailed", "ManagedLabelFalse", "FinalizerCheckFailed",
            "CreationTimedOut", "UpdateTimedOut", "DeletionTimedOut", "LabelRemovalTimedOut")
AFTER_WAIT = {"CreationTimedOut": "OK", "UpdateTimedOut": "OK", "DeletionTimedOut": "WaitingForRemoval",
              "LabelRemovalTimedOut": ""}
VERSIONS = ("gen:1", "gen:2", "gen:7", "gen:+5", "gen:05", "gen:", "gen:x", "gen:9223372036854775808",
            "gen:-9223372036854775808", "rv:1", "rv:22", "rv:", "x")


def names(n):
    return ["c%05d" % i for i in range(n)]


def obj(records=None, selected=None, status=None, stored_version=None, generation=0, collision=None,
        resources_updated=False, template="t1", override="o1", reason="", nnf=False):
    records = records or {}
    return {"status": status, "generation": generation, "collision": collision,
            "selected": list(records) if selected is None else selected, "records": records,
            "resources_updated": resources_updated, "stored_version": stored_version, "template": template,
            "override": override, "reason": reason, "nnf": nnf}


def stored(pairs, template="t1", override="o1"):
    """A stored PropagatedVersion status; ``pairs`` None: the list is absent."""
    s = {"templateVersion": template, "overrideVersion": override}
    if pairs is not None:
        s["clusterVersions"] = [{"clusterName": n, "version": v} for n, v in pairs]
    return s


def cond(status="True", reason=""):
    c = {"type": "Propagation", "status": status, "lastTransitionTime": "T0", "lastUpdateTime": "U0"}
    if reason:
        c["reason"] = reason
    return c


def settled_status(o, conditions=None):
    """The stored status that leaves o unchanged: what the reference would write for it, with a condition."""
    st = {k: v for k, v in R.finish({**o, "status": None})["status"].items() if k in ("clusters", "syncedGeneration", "collisionCount")}
    r = R.finish({**o, "status": None})["reason"]
    st["conditions"] = conditions if conditions is not None else [cond("True" if r == "" else "False", r)]
    return st


def named():
    """name → (cluster names, objects)."""
    n = names(8)
    a, b, c, d = n[:4]
    ok = {a: ("UpdateTimedOut", "gen:2"), b: ("CreationTimedOut", "rv:5")}
    out = {}
    base = obj(dict(ok))
    out["empty_object"] = [obj()]
    out["empty_sel"] = [obj(dict(ok), selected=[], stored_version=stored([(a, "gen:2"), (c, "gen:1")]))]
    out["all_label_removal"] = [obj({a: ("LabelRemovalTimedOut", ""), b: ("LabelRemovalTimedOut", "")}, selected=[],
                                    resources_updated=True, status={"conditions": [cond()]})]
    out["wait_transitions"] = [obj({a: ("CreationTimedOut", "gen:1"), b: ("UpdateTimedOut", "rv:1"), c: ("DeletionTimedOut", ""),
                                    d: ("LabelRemovalTimedOut", "")}, selected=[a, b])]
    out["oldv_disjoint"] = [obj(dict(ok), selected=n, stored_version=stored([(c, "gen:1"), (d, "rv:9")]))]
    out["oldv_equal"] = [obj(dict(ok), stored_version=stored([(a, "gen:2"), (b, "rv:5")]))]
    out["oldv_equal_other_version"] = [obj(dict(ok), stored_version=stored([(a, "gen:2"), (b, "rv:6")]))]
    out["oldv_interleaved"] = [obj({b: ("UpdateTimedOut", "gen:2"), d: ("UpdateFailed", ""), n[5]: ("UpdateTimedOut", "rv:1")},
                                   selected=n, stored_version=stored([(a, "gen:1"), (b, "gen:1"), (c, "rv:3"), (d, "rv:4"), (n[6], "gen:7")]))]
    out["oldv_unselected_dropped"] = [obj(dict(ok), selected=[a, b], stored_version=stored([(a, "gen:2"), (b, "rv:5"), (c, "gen:1")]))]
    out["oldv_not_current"] = [obj(dict(ok), selected=n, stored_version=stored([(a, "gen:2"), (b, "rv:5"), (c, "gen:1")], template="t0"))]
    out["oldv_nil_and_empty"] = [obj({a: ("ClusterNotReady", "")}, stored_version=stored(None)),
                                 obj({a: ("ClusterNotReady", "")}, stored_version=stored([])),
                                 obj(dict(ok), stored_version=stored(None)), obj(dict(ok), stored_version=stored([]))]
    out["oldv_irregular"] = [obj(dict(ok), selected=n, stored_version=stored([(b, "rv:5"), (a, "gen:2")])),
                             obj(dict(ok), selected=n, stored_version=stored([(a, "gen:2"), (a, "gen:1"), (b, "rv:5")])),
                             obj({a: ("UpdateFailed", "")}, selected=n, stored_version=stored([(a, "gen:3"), (a, "gen:1")])),
                             obj(dict(ok), selected=n, stored_version=stored([(a, "gen:2"), (b, "rv:5"), ("zz-not-joined", "gen:1")])),
                             obj(dict(ok), selected=n, stored_version=stored([(a, "gen:2"), (b, "rv:5"), (c, "")]))]
    # the generation map is counted apart from the status map: a ClusterNotReady cluster has a status and no version
    quirk = obj({a: ("UpdateTimedOut", "gen:2"), b: ("ClusterNotReady", "")})
    out["generation_map_length"] = [{**quirk, "status": settled_status(quirk)}]
    unparsed = obj({a: ("UpdateTimedOut", "gen:x"), b: ("UpdateTimedOut", "gen:9223372036854775808")})
    out["generation_unparsed"] = [{**unparsed, "status": settled_status(unparsed)}]
    out["unchanged"] = [{**base, "status": settled_status(base)}]
    out["unchanged_resources_updated"] = [{**base, "status": settled_status(base), "resources_updated": True}]
    out["resources_updated_empty_map"] = [obj({a: ("LabelRemovalTimedOut", "")}, resources_updated=True,
                                              status={"conditions": [cond()]})]
    st = settled_status(base)
    out["olds_status_differs"] = [{**base, "status": {**st, "clusters": [dict(st["clusters"][0], status="UpdateFailed"), st["clusters"][1]]}}]
    out["olds_generation_differs"] = [{**base, "status": {**st, "clusters": [dict(st["clusters"][0], generation=1), st["clusters"][1]]}}]
    out["olds_other_cluster"] = [{**base, "status": {**st, "clusters": [st["clusters"][0], dict(st["clusters"][1], name=c)]}}]
    out["olds_unordered"] = [{**base, "status": {**st, "clusters": st["clusters"][::-1]}}]
    out["scalars"] = [{**base, "status": st, "generation": 3}, {**base, "status": st, "collision": 0},
                      {**base, "status": {**st, "collisionCount": 1, "syncedGeneration": 4}, "collision": 1, "generation": 4}]
    trans = []
    failed = obj({a: ("UpdateFailed", "")})
    for o in (base, failed, {**base, "nnf": True}, {**base, "reason": "ComputePlacementFailed"}):
        for conds in (None, [], [cond("True")], [cond("False", "CheckClusters")], [cond("False", "NamespaceNotFederated")],
                      [cond("True", "CheckClusters")], [cond("False")], [cond("Unknown")], [cond("False", "SomethingElse")],
                      [{"type": "Other", "status": "True"}, cond("True")]):
            s = settled_status(o)
            if conds is None:
                del s["conditions"]
            else:
                s["conditions"] = conds
            trans.append({**o, "status": s})
    out["condition_transitions"] = trans
    irregular = {**base, "status": {**st, "clusters": [st["clusters"][0], st["clusters"][0]]}}
    out["status_on_host_between"] = [{**base, "status": st}, irregular, {**failed, "status": settled_status(failed)},
                                     {**base, "status": {**st, "clusters": [st["clusters"][0], {"name": "zz-not-joined", "status": "OK"}]}},
                                     {**base, "status": {**st, "clusters": [st["clusters"][0], {"name": b, "status": "Odd"}]}},
                                     {**base, "status": {**st, "clusters": [st["clusters"][0], {"name": b}]}}]
    # the last object's versions fill its capacity: every record has a version, every stored one is retained
    out["ends_at_capacity"] = [base, obj(dict(ok), selected=n, stored_version=stored([(c, "gen:1"), (d, "rv:9")]),
                                         status=None)]
    return {k: (n, v) for k, v in out.items()}


def random_object(rng, cl, size, irregular=False):
    """One object over the cluster names ``cl`` with about ``size`` entries in each list."""
    size = min(size, len(cl))
    ent = rng.sample(cl, size)
    records = {}
    mode = rng.randrange(4)
    for name in ent:
        s = rng.choice(STATUSES) if mode == 0 else rng.choice(("UpdateTimedOut", "CreationTimedOut", "UpdateTimedOut", "UpdateFailed",
                                                               "ClusterNotReady", "DeletionTimedOut", "LabelRemovalTimedOut"))
        if mode == 3:
            s = rng.choice(("UpdateTimedOut", "CreationTimedOut"))
        v = rng.choice(VERSIONS if rng.random() < 0.2 else ("gen:1", "gen:2", "rv:22")) if s in ("UpdateTimedOut", "CreationTimedOut") \
            and rng.random() < 0.9 else ""
        records[name] = (s, v)
    others = [n for n in cl if n not in records]
    selected = [n for n in ent if rng.random() < 0.8] + rng.sample(others, min(len(others), rng.randrange(size + 2)))
    o = obj(records, selected, generation=rng.choice((0, 1, 5)), collision=rng.choice((None, 0, 2)),
            resources_updated=rng.random() < 0.3, nnf=rng.random() < 0.1, reason="" if rng.random() < 0.9 else "PlanRolloutFailed")
    # the stored versions
    vm = rng.randrange(6)
    if vm:
        pairs = []
        for name in sorted(rng.sample(cl, size)):
            v = records.get(name, ("", ""))[1]
            pairs.append((name, v if v and rng.random() < 0.7 else rng.choice(("gen:1", "gen:3", "rv:22"))))
        if vm == 1:  # what the reference would store: nothing to write
            pairs = [(c["clusterName"], c["version"]) for c in R.finish(o)["version_status"]["clusterVersions"]]
        o["stored_version"] = stored(None if vm == 2 and rng.random() < 0.5 else pairs, template="t0" if vm == 3 else "t1")
        if irregular and o["stored_version"].get("clusterVersions"):
            o["stored_version"]["clusterVersions"].append({"clusterName": pairs[0][0], "version": "gen:9"})
    # the stored status
    sm = rng.randrange(6)
    if sm:
        st = settled_status(o)
        cls = st.get("clusters", [])
        if sm == 2 and cls:
            k = rng.randrange(len(cls))
            cls[k] = dict(cls[k], status="UpdateFailed" if cls[k]["status"] != "UpdateFailed" else "OK")
        elif sm == 3 and cls:
            k = rng.randrange(len(cls))
            cls[k] = dict(cls[k], generation=cls[k].get("generation", 0) + 1)
        elif sm == 4 and cls:
            del cls[rng.randrange(len(cls))]
        elif sm == 5:
            st["conditions"] = rng.choice(([], [cond("True")], [cond("False", "CheckClusters")], [cond("False", "NamespaceNotFederated")]))
        if irregular and cls:
            cls.append(dict(cls[0]))
        if cls:
            st["clusters"] = cls
        o["status"] = st
    return o


def random_batch(seed, n_clusters, n_objects, max_size, irregular_every=0):
    """(cluster names in a shuffled order, objects). ``irregular_every`` > 0: every that-many-th object gets stored
    lists with a duplicate; never otherwise."""
    rng = random.Random(seed)
    cl = names(n_clusters)
    objs = [random_object(rng, cl, rng.randrange(max_size + 1), bool(irregular_every) and k % irregular_every == irregular_every - 1)
            for k in range(n_objects)]
    order = list(cl)
    rng.shuffle(order)
    return order, objs


def sized_batch(seed, n_clusters, sizes):
    rng = random.Random(seed)
    cl = names(n_clusters)
    return cl, [random_object(rng, cl, s) for s in sizes]


def is_on_host(o, joined):
    """The declared deviation, decided from the dicts alone: a stored status.clusters with a duplicate name, a cluster
    that is not joined or a status outside the constants."""
    seen = set()
    for c in (o["status"] or {}).get("clusters") or []:
        if c.get("name") in seen or c.get("name") not in joined or c.get("status", "") not in STATUSES:
            return True
        seen.add(c.get("name"))
    return False


def pack(cluster_names, objs):
    from kubeadmiral_amd import syncfin as SF
    b = SF.SyncFinishBatch(cluster_names)
    for o in objs:
        b.add(o["status"], o["generation"], o["collision"], o["selected"], o["records"], o["resources_updated"],
              o["stored_version"], o["template"], o["override"], o["reason"], o["nnf"])
    return b


def compare(batch, result, objs, now=R.NOW):
    """None, or the first difference between ``result`` mapped through apply and syncfin_ref.finish."""
    for k, (got, o) in enumerate(zip(batch.apply(result, now), objs)):
        want = R.finish(o, now)
        for field in ("version_status", "version_write", "status_write", "reason", "clusters_changed"):
            if getattr(got, field) != want[field]:
                return k, field, getattr(got, field), want[field]
        if want["status_write"] and got.status != want["status"]:
            return k, "status", got.status, want["status"]
    return None


# ---------------------------------------------------------------------- update rows
def member(generation=0, rv="7", replicas=None, surge=None, unavailable=None, labels=None, name="x"):
    m = {"metadata": {"name": name, "namespace": "ns", "resourceVersion": rv}, "spec": {}}
    if generation:
        m["metadata"]["generation"] = generation
    if labels is not None:
        m["metadata"]["labels"] = labels
    if replicas is not None:
        m["spec"]["replicas"] = replicas
    ru = {k: v for k, v in (("maxSurge", surge), ("maxUnavailable", unavailable)) if v is not None}
    if ru:
        m["spec"]["strategy"] = {"rollingUpdate": ru}
    return m


def update_rows(seed, n_clusters, n_objects, rows_per_object):
    """(cluster names, per object (stored version status, template, override), rows (object, cluster, desired, member))."""
    rng = random.Random(seed)
    cl = names(n_clusters)
    objects, rows = [], []
    for k in range(n_objects):
        rec = sorted(rng.sample(cl, min(len(cl), rng.randrange(rows_per_object + 2))))
        mode = rng.randrange(4)
        st = None if mode == 0 else stored([(n, rng.choice(("gen:2", "rv:7", "gen:3"))) for n in rec], template="t0" if mode == 1 else "t1")
        objects.append((st, "t1", "o1"))
        for name in rng.sample(cl, min(len(cl), rows_per_object)):
            m = member(rng.choice((0, 2, 3)), "7", rng.choice((None, 1, 2)), rng.choice((None, "25%", 1)), rng.choice((None, "25%", 1)),
                       rng.choice((None, {}, {"a": "b"})))
            d = member(0, "", rng.choice((None, 1, 2)), rng.choice((None, "25%", 1, 1.5)), rng.choice((None, "25%", 1)),
                       rng.choice((None, {}, {"a": "b"})))
            if rng.random() < 0.6:  # a desired object that agrees with the member: the version decides
                d = {"metadata": {k2: v for k2, v in m["metadata"].items() if k2 in ("name", "namespace", "labels")},
                     "spec": json.loads(json.dumps(m["spec"]))}
            rows.append((k, name, d, m))
    return cl, objects, rows


def pack_rows(cluster_names, objects, rows, replicas_spec="spec.replicas"):
    from kubeadmiral_amd import syncfin as SF
    b = SF.SyncFinishBatch(cluster_names)
    for st, t, o in objects:
        b.add_versions(st, t, o)
    for k, name, d, m in rows:
        b.add_update(k, name, d, m, replicas_spec)
    return b


def compare_rows(batch, result, objects, rows, replicas_spec="spec.replicas"):
    got = batch.apply_needs_update(result)
    for k, name, d, m in rows:
        rec = R.version_get(*objects[k]).get(name, "")
        want = (R.needs_update(d, m, rec, replicas_spec), rec)
        if got[k][name] != want:
            return k, name, got[k][name], want
    return None


def golden():
    with open(os.path.join(os.path.dirname(__file__), "golden", "syncfin.json")) as f:
        return json.load(f)
