"""Batched reconcile: the scheduler controller's per-object loop, one GPU pass per batch.

``Scheduler.reconcile`` (pkg/controllers/scheduler/scheduler.go:240-309) runs
per federated object on ``--worker-count`` goroutines: look up the policy and
profile (``prepareToSchedule``, :311-443), compute the scheduling-trigger hash
and skip the object if it is unchanged (:394-421), build the SchedulingUnit and
call ``ScheduleAlgorithm.Schedule`` (``schedule``, :445-521), then write the
result back (``applySchedulingResult``, :632-695). :class:`BatchReconciler`
takes a whole batch of objects through the same steps with the two hot
stages batched on the GPU — every object's trigger hash in one
``kad_trigger_run`` and every SchedulingUnit of one framework in one
``kad_schedule`` — and returns, per object, what the reference's reconcile
would have done (worker status, whether it scheduled, whether the object
changed). Objects are mutated in place exactly as the reference mutates its
deep copy before ``Update``.

Out of scope (no API server here): pending-controller bookkeeping
(``pendingcontrollers``), events, the ``Update`` call itself, webhook plugins
(rejected by :class:`~kubeadmiral_amd.framework.Framework`), deletion
timestamps. Policies and profiles are looked up in the dicts the caller passes
(the informer caches of the reference).
"""

from __future__ import annotations

from dataclasses import dataclass
from typing import Dict, List, Optional, Sequence, Tuple

from . import framework as F
from . import objects as O
from . import types as T
from .pack import ST_NO_FEASIBLE
from .runtime import BatchScheduler, Context, TriggerHasher

STATUS_ALL_OK = "AllOK"   # worker.StatusAllOK
STATUS_ERROR = "Error"    # worker.StatusError


@dataclass
class StatusAggOutcome:
    """One source object's outcome of :meth:`BatchReconciler.reconcile_status_aggregation`."""
    status: str              # STATUS_ALL_OK / STATUS_ERROR
    need_update: bool        # the plugin's needUpdate: the source object was written and is to be updated
    error: Optional[str]     # the reference's error return


@dataclass
class ReconcileOutcome:
    status: str                                  # STATUS_ALL_OK / STATUS_ERROR
    stage: str = ""                              # where the reconcile ended (see BatchReconciler.reconcile)
    scheduled: bool = False                      # a result was computed and applied
    modified: bool = False                       # applySchedulingResult changed the object
    result: Optional[T.ScheduleResult] = None
    error: str = ""
    diagnosis: str = ""                          # reconcile(explain=True): why no cluster was feasible


class BatchReconciler:
    """Scheduler.reconcile for a batch of federated objects of one FederatedTypeConfig."""

    def __init__(self, type_config: O.FederatedTypeConfig, ctx: Optional[Context] = None, device: int = 0,
                 native_objects: bool = True):
        """``native_objects``: SchedulingUnits built and results applied by the library (kad_units_from_objects /
        kad_apply_results, include/kad_objects.h) over the objects' JSON, instead of objects.py per object."""
        self.type_config = type_config
        self.native_objects = native_objects
        self.ctx = ctx if ctx is not None else Context(device)
        self.hasher = TriggerHasher(self.ctx)
        self.scheduler = BatchScheduler(self.ctx)
        self._clusters_key = None
        self._pass = None  # the batch the last reconcile left resident (last_pass)
        self.policy_refs = None  # policyrc.PolicyRefCounter, from the first reconcile_policy_refcounts on
        self.meters = None  # monitor.MeterTable, from the first reconcile_monitor / monitor_report on

    def _framework(self, profile: Optional[dict]) -> F.Framework:
        """createFramework (scheduler.go:492, profile.go:52-82): default plugins + the profile's changes."""
        return F.Framework(F.apply_profile(F.default_enabled_plugins(), profile))

    def reconcile(self, objs: Sequence[dict], policies: Dict[Tuple[str, str], O.PropagationPolicy],
                  clusters: List[T.FederatedCluster], profiles: Optional[Dict[str, Optional[dict]]] = None,
                  explain: bool = False) -> List[ReconcileOutcome]:
        """Reconcile every object against the joined ``clusters``.

        ``policies`` maps (namespace, name) → policy ("" namespace for
        ClusterPropagationPolicies); ``profiles`` maps SchedulingProfile name →
        its ``spec.plugins`` dict (None = no changes). Stages recorded in
        ``ReconcileOutcome.stage``: ``policy-not-found``, ``profile-not-found``,
        ``trigger-error``, ``unchanged`` (trigger hash equal), ``no-scheduling``,
        ``unit-error``, ``framework-error``, ``schedule-error``, ``apply-error``,
        ``scheduled``. ``explain``: every object scheduled with no feasible cluster gets
        ``ReconcileOutcome.diagnosis``, the per-plugin rejection counts of its unit
        (``FilterDiagnosis.message``), from one kad_explain per framework batch over just those units.
        """
        profiles = profiles or {}
        self._pass = None
        out: List[Optional[ReconcileOutcome]] = [None] * len(objs)
        why: Dict[int, str] = {}
        ctx_pol: List[Optional[O.PropagationPolicy]] = [None] * len(objs)
        ctx_prof: List[Optional[str]] = [None] * len(objs)

        # prepareToSchedule :349-392 — policy and profile lookup
        live = []
        for i, obj in enumerate(objs):
            key = O.matched_policy_key(obj, self.type_config.namespaced)
            if key is not None:
                pol = policies.get(key)
                if pol is None:
                    out[i] = ReconcileOutcome(STATUS_ALL_OK, "policy-not-found")
                    continue
                ctx_pol[i] = pol
                name = pol.spec.scheduling_profile
                if name:
                    if name not in profiles:
                        out[i] = ReconcileOutcome(STATUS_ALL_OK, "profile-not-found")
                        continue
                    ctx_prof[i] = name
            live.append(i)

        # :394-421 — trigger hashes for the whole batch in one GPU pass
        key = T.clusters_fingerprint(clusters)  # content (labels, taints, API resources), not the list object
        if key != self._clusters_key:
            self.hasher.set_clusters(clusters)
            self._clusters_key = key
        hashed, prefixes = [], []
        for i in live:
            try:
                prefixes.append(O.trigger_prefix(self.type_config, objs[i], ctx_pol[i]))
                hashed.append(i)
            except O.ObjectError as e:
                out[i] = ReconcileOutcome(STATUS_ERROR, "trigger-error", error=str(e))
        self.ctx.trigger_prefixes_upload(prefixes)
        self.ctx.trigger_run()
        hashes = self.ctx.trigger_download()
        to_schedule = []
        for i, h in zip(hashed, hashes.tolist()):
            changed = O.add_annotation(objs[i], O.SCHEDULING_TRIGGER_HASH_ANNOTATION, O.format_trigger_hash(h))
            if not changed:
                out[i] = ReconcileOutcome(STATUS_ALL_OK, "unchanged")
            elif (O.get_annotations(objs[i]) or {}).get(O.NO_SCHEDULING_ANNOTATION, ""):
                out[i] = ReconcileOutcome(STATUS_ALL_OK, "no-scheduling")
            else:
                to_schedule.append(i)

        if self.native_objects:
            self._schedule_and_apply_native(objs, to_schedule, ctx_pol, ctx_prof, profiles, clusters, out,
                                            why if explain else None)
            return out  # type: ignore[return-value]

        # schedule :445-521 — units grouped by framework, one GPU batch per framework
        results: Dict[int, T.ScheduleResult] = {}
        groups: Dict[Optional[str], List[Tuple[int, T.SchedulingUnit]]] = {}
        for i in to_schedule:
            if ctx_pol[i] is None:
                results[i] = T.ScheduleResult({})  # :454-467 no policy: schedule to no clusters
                continue
            try:
                su = O.scheduling_unit_for_fed_object(self.type_config, objs[i], ctx_pol[i])
            except (O.ObjectError, O.GoPanic) as e:
                out[i] = ReconcileOutcome(STATUS_ERROR, "unit-error", error=str(e))
                continue
            groups.setdefault(ctx_prof[i], []).append((i, su))
        for prof_name, members in groups.items():
            try:
                fwk = self._framework(profiles.get(prof_name) if prof_name else None)
            except F.FrameworkError as e:
                for i, _ in members:
                    out[i] = ReconcileOutcome(STATUS_ERROR, "framework-error", error=str(e))
                continue
            res = self.scheduler.schedule(fwk, [su for _, su in members], clusters)
            if explain:  # ScheduleResult(None) is the NO_FEASIBLE unit's result (results.to_schedule_result)
                self._explain(fwk, [(i, w) for w, ((i, _), r) in enumerate(zip(members, res))
                                    if isinstance(r, T.ScheduleResult) and r.suggested_clusters is None], why)
            for (i, _), r in zip(members, res):
                if isinstance(r, T.ScheduleError):
                    out[i] = ReconcileOutcome(STATUS_ERROR, "schedule-error", error=str(r))
                else:
                    results[i] = r

        # reconcile :291-308 + persistSchedulingResult → applySchedulingResult
        for i, r in results.items():
            pol = ctx_pol[i]
            follower = False
            threshold = None
            try:
                if pol is not None:
                    follower = not pol.spec.disable_follower_scheduling
                    am = pol.spec.auto_migration
                    if am is not None:
                        if am.when.pod_unschedulable_for is None:
                            raise O.GoPanic("invalid memory address or nil pointer dereference")  # :302
                        threshold = O.parse_duration(am.when.pod_unschedulable_for)
                modified = O.apply_scheduling_result(self.type_config, objs[i], r, follower, threshold)
            except (O.ObjectError, O.GoPanic) as e:
                out[i] = ReconcileOutcome(STATUS_ERROR, "apply-error", result=r, error=str(e))
                continue
            out[i] = ReconcileOutcome(STATUS_ALL_OK, "scheduled", True, modified, r, diagnosis=why.get(i, ""))
        return out  # type: ignore[return-value]

    def _explain(self, fwk: F.Framework, pairs: List[Tuple[int, int]], why: Dict[int, str]) -> None:
        """``why[i]`` = the filter diagnosis of unit w of the batch just scheduled, for (object i, unit w) pairs."""
        if not pairs:
            return
        d = self.ctx.explain(fwk, [w for _, w in pairs])
        for k, (i, _) in enumerate(pairs):
            why[i] = d.message(k)

    # ------------------------------------------------------------------ the native object path
    @staticmethod
    def _apply_params(pol):
        """(follower, threshold ns) of reconcile :291-308; raises like the reference."""
        if pol is None:
            return False, None
        threshold = None
        am = pol.spec.auto_migration
        if am is not None:
            if am.when.pod_unschedulable_for is None:
                raise O.GoPanic("invalid memory address or nil pointer dereference")  # :302
            threshold = O.parse_duration(am.when.pod_unschedulable_for)
        return not pol.spec.disable_follower_scheduling, threshold

    def _schedule_and_apply_native(self, objs, to_schedule, ctx_pol, ctx_prof, profiles, clusters, out, why=None):
        """The schedule and apply stages over the objects' JSON: per framework one kad_units_from_objects, one
        packed GPU batch, then one kad_apply_results for every object with a result."""
        import json

        from . import columns as K
        from .results import to_schedule_result_cols

        results: Dict[int, T.ScheduleResult] = {}
        groups: Dict[Optional[str], List[int]] = {}
        for i in to_schedule:
            if ctx_pol[i] is None:
                results[i] = T.ScheduleResult({})  # :454-467 no policy: schedule to no clusters
                continue
            groups.setdefault(ctx_prof[i], []).append(i)
        pol_index: Dict[int, int] = {}
        pol_json: List[dict] = []
        for i in to_schedule:
            if ctx_pol[i] is not None and id(ctx_pol[i]) not in pol_index:
                pol_index[id(ctx_pol[i])] = len(pol_json)
                pol_json.append(O.policy_to_json(ctx_pol[i]))
        pol_text = [json.dumps(p) for p in pol_json]
        names: List[str] = []
        for prof_name, members in groups.items():
            try:
                fwk = self._framework(profiles.get(prof_name) if prof_name else None)
            except F.FrameworkError as e:
                for i in members:
                    out[i] = ReconcileOutcome(STATUS_ERROR, "framework-error", error=str(e))
                continue
            built = K.units_from_objects(self.type_config, [json.dumps(objs[i]) for i in members], pol_text,
                                         [pol_index[id(ctx_pol[i])] for i in members])
            ok = []
            for k, i in enumerate(members):
                if built.status[k] == K.OBJ_OK:
                    ok.append((i, int(built.unit_index[k])))
                else:
                    out[i] = ReconcileOutcome(STATUS_ERROR, "unit-error", error=built.messages[k])
            if not ok:
                continue
            res, snap = self.scheduler.schedule_columns(fwk, built.cols, clusters)
            names = snap.names
            self._record_pass(len(res.status), ok, out)
            if why is not None:
                self._explain(fwk, [(i, w) for i, w in ok if int(res.status[w]) == ST_NO_FEASIBLE], why)
            for i, w in ok:
                r = to_schedule_result_cols(res, w, built.cols, names)
                if isinstance(r, T.ScheduleError):
                    out[i] = ReconcileOutcome(STATUS_ERROR, "schedule-error", error=str(r))
                else:
                    results[i] = r

        # reconcile :291-308 + persistSchedulingResult → applySchedulingResult, one native pass
        todo, follower, threshold = [], [], []
        for i, r in sorted(results.items()):
            try:
                f, t = self._apply_params(ctx_pol[i])
            except (O.ObjectError, O.GoPanic) as e:
                out[i] = ReconcileOutcome(STATUS_ERROR, "apply-error", result=r, error=str(e))
                continue
            todo.append(i)
            follower.append(f)
            threshold.append(t)
        if not todo:
            return
        table = list(names)
        at = {n: k for k, n in enumerate(table)}
        off, cl, rep = [0], [], []
        for i in todo:
            for n, v in (results[i].suggested_clusters or {}).items():
                if n not in at:  # a sticky result's cluster that left the snapshot
                    at[n] = len(table)
                    table.append(n)
                cl.append(at[n])
                rep.append(-1 if v is None else v)
            off.append(len(cl))
        st, modified, texts, msgs, fields = K.apply_results(self.type_config, [json.dumps(objs[i]) for i in todo],
                                                            table, off, cl, rep, follower, threshold, with_fields=True)
        for k, i in enumerate(todo):
            r = results[i]
            if st[k] != K.APPLY_OK:
                out[i] = ReconcileOutcome(STATUS_ERROR, "apply-error", result=r, error=msgs[k])
                continue
            if modified[k]:  # the written fields are set in place, as the reference mutates its deep copy
                for (a, b), v in zip(K.APPLY_FIELDS, fields[k]):
                    if v is not None:
                        objs[i].setdefault(a, {})[b] = json.loads(v)
            out[i] = ReconcileOutcome(STATUS_ALL_OK, "scheduled", True, bool(modified[k]), r,
                                      diagnosis=(why or {}).get(i, ""))

    # ------------------------------------------------------------------ follower scheduling
    def _record_pass(self, n_units: int, ok: List[Tuple[int, int]], out: list) -> None:
        """The batch now resident on the device: (its unit count, (object index, unit) pairs, the outcome list
        the reconcile goes on filling in) — what :attr:`last_pass` is computed from."""
        self._pass = (n_units, list(ok), out)

    @property
    def last_pass(self) -> Optional[List[int]]:
        """What :meth:`reconcile_followers` takes as ``resident`` after the last :meth:`reconcile` /
        :meth:`reconcile_texts`: per unit w of the batch that pass left resident on the device, the index (in
        the reconciled sequence) of the object whose scheduler placement that unit's device result describes,
        -1 for none; None when the pass scheduled nothing (whatever is resident belongs to an earlier pass).
        A unit describes its object when the result was applied (stage ``scheduled``) or when Schedule failed
        (``schedule-error``: the device status is an error class, for which the follower union reads the
        placement the object keeps). Objects whose apply failed keep their old placement although their unit
        is OK on the device: they are left out, and read from their dicts like every leader outside the batch."""
        if self._pass is None:
            return None
        n_units, ok, out = self._pass
        units = [-1] * n_units
        for i, w in ok:
            if out[i] is not None and out[i].stage in ("scheduled", "schedule-error"):
                units[w] = i
        return units

    def reconcile_followers(self, leaders: Sequence[dict], followers: Sequence[dict],
                            clusters: List[T.FederatedCluster], resident: Optional[Sequence[int]] = None,
                            source_to_federated=None):
        """The follower controller's two reconciles for a batch (pkg/controllers/follower/controller.go):
        every leader's followers are inferred (reconcileLeader :285-311), then every follower dict gets
        ``spec.follows`` and the union of its leaders' placements (reconcileFollower :463-483, updateFollower),
        in place, with the unions and SetPlacementNames' change test in one kad_follower_union.

        ``leaders``: federated leader dicts as they stand after their own reconcile. ``resident``:
        ``self.last_pass`` of the :meth:`reconcile` / :meth:`reconcile_texts` just run over the same sequence —
        those leaders' scheduler placements are then read from the results still on the device (resident
        mode: OK and sticky units from their slots, error units from the placement the object keeps), the
        other leaders' and every other controller's placements from the dicts; None: every placement from the
        dicts (explicit mode). Returns (needs_update per follower, {leader index: error} for the leaders whose
        followers could not be inferred — they contribute no followers, as a reconcile that ends in
        StatusError leaves the cache)."""
        from . import follower as FL

        s2f = source_to_federated if source_to_federated is not None else FL.default_source_to_federated()
        index = FL.FollowerIndex()
        errors: Dict[int, str] = {}
        refs = [FL.leader_reference(ld) for ld in leaders]
        for i, ld in enumerate(leaders):
            try:
                index.update_leader(refs[i], FL.infer_followers(ld, FL.source_group_kind(ld), s2f))
            except FL.FollowerError as e:
                errors[i] = str(e)
        frefs = [FL.follower_reference(f) for f in followers]
        for fr, f in zip(frefs, followers):
            index.observe_follower(fr, f)
        if resident is None:
            snap = self.scheduler.set_clusters(clusters)
            order = list(range(len(leaders)))
            args = {"leaders": [FL.placement_names(leaders[i]) for i in order]}
        else:
            snap = self.ctx.snap  # the snapshot the resident batch was scheduled against
            W = len(resident)
            rest = sorted(set(range(len(leaders))) - set(resident))
            order = list(resident) + rest
            sched_name = O.PREFIXED_GLOBAL_SCHEDULER_NAME
            keep, sched = [], []
            for k, i in enumerate(order):
                if i < 0:
                    names = own = []
                elif k < W:
                    own = FL.placement_names(leaders[i], sched_name) or []
                    # the device reads the unit's result; it lacks what other controllers placed and, for a
                    # sticky unit, the current clusters that left the snapshot
                    names = FL.placement_names(leaders[i], None, exclude=sched_name) + \
                        [n for n in own if n not in snap.name_id]
                else:
                    own, names = [], FL.placement_names(leaders[i])
                keep.append(names)
                if k < W:
                    sched.append(own)
            args = {"leaders": None, "keep": keep, "sched": sched, "n_leaders": len(order)}
        leader_index = {refs[i]: k for k, i in enumerate(order) if i >= 0}
        fol_off, fol_leader, desired = index.csr(frefs, leader_index)
        placer = FL.FollowerPlacer(self.ctx, snap)
        return placer.apply(followers, desired, fol_off, fol_leader, **args), errors

    # ------------------------------------------------------------------ auto migration
    def reconcile_auto_migration(self, objs: Sequence[dict], cluster_objs: Sequence[Sequence[Tuple[str, dict]]],
                                 pods: Sequence[Sequence], now_ns: int,
                                 clusters: Optional[List[T.FederatedCluster]] = None):
        """The auto-migration controller's reconcile for a batch
        (pkg/controllers/automigration/controller.go:178-290): ``cluster_objs[i]`` are object i's (cluster name,
        member-cluster object) pairs, ``pods[i][j]`` the pod dicts of pair j or an exception object for a listing
        that failed (automigration.PodListError). Objects without a parseable threshold annotation lose the
        info annotation on the host (:217-224); the others are counted and compared in one
        kad_migrate_estimate and only the changed ones get the annotation rewritten, in place.

        The cluster ids are those of the resident snapshot (``clusters``: upload these first; None: the
        snapshot the last reconcile left). Returns, per object, (result, estimatedCapacity, needsUpdate):
        result is None (worker.StatusAllOK) or (retry_after_ns or None, backoff); estimatedCapacity is None
        for a disabled object."""
        from . import automigration as AM

        snap = self.scheduler.set_clusters(clusters) if clusters is not None else self.ctx.snap
        if snap is None:
            raise ValueError("no snapshot is resident: pass clusters")
        batch = AM.MigrationBatch(self.type_config, snap.names, now_ns)
        out: list = [None] * len(objs)
        members = []
        for i, obj in enumerate(objs):
            thr = AM.threshold_of(obj)
            if thr is None:
                out[i] = (None, None, AM.apply(obj, None, enabled=False))
            else:
                batch.add(obj, thr, cluster_objs[i], pods[i])
                members.append(i)
        if members:
            r = self.ctx.migrate_estimate(**batch.arrays())
            updated = batch.apply([objs[i] for i in members], r)
            for k, i in enumerate(members):
                out[i] = (batch.result(r, k), batch.capacities(r, k), updated[k])
        return out

    # ------------------------------------------------------------------ cluster status
    def reconcile_cluster_status(self, clusters: List[T.FederatedCluster], cluster_nodes: Sequence[Sequence[dict]],
                                 cluster_pods: Sequence[Sequence[dict]], objs: Optional[Sequence[dict]] = None
                                 ) -> List[str]:
        """The federated-cluster controller's resource collection for a batch of member clusters
        (pkg/controllers/federatedcluster/clusterstatus.go:162-202): ``cluster_nodes[i]`` / ``cluster_pods[i]``
        are the node and pod dicts listed from ``clusters[i]``. One kad_cluster_resources sums them (clusters
        outside the device's number domain on the host, clusterstatus.ClusterStatusBatch), the clusters whose
        resources changed in value are replaced in ``clusters`` (in place) by copies with the new ``allocatable``
        / ``available``, ``objs[i]`` (FederatedCluster dicts, optional) get ``status.resources``, and the resident
        snapshot follows: a kad_snapshot_update of the changed columns, a repack where the delta cannot express
        the change, nothing when no cluster changed. Returns the names of the changed clusters."""
        from . import clusterstatus as CS

        batch = CS.ClusterStatusBatch()
        for nodes, pods in zip(cluster_nodes, cluster_pods):
            batch.add(nodes, pods)
        arrays = batch.arrays()
        r = self.ctx.cluster_resources(**arrays) if batch.device else None
        new, changed = batch.apply(r, clusters, objs)
        clusters[:] = new
        self.scheduler.set_clusters(clusters)
        return changed

    # ------------------------------------------------------------------ status aggregation
    def reconcile_status_aggregation(self, sources: Sequence[dict], fed_objects: Sequence[Optional[dict]],
                                     cluster_objs: Sequence[Dict[str, dict]], now: Optional[int] = None
                                     ) -> List[StatusAggOutcome]:
        """The status aggregator's reconcile for a batch of source objects
        (pkg/controllers/statusaggregator/controller.go:249-348): ``sources[i]`` is a Deployment or a Job (by its
        ``kind``), ``fed_objects[i]`` its federated object and ``cluster_objs[i]`` its copies in the ready member
        clusters (cluster name → object). One kad_status_aggregate per kind folds the members' statuses
        (statusagg.StatusAggBatch: objects outside the device's time domain on the host); the source objects
        whose status or digests annotation changed are written in place, the others stay untouched. ``now``
        (Unix seconds, default the clock) stamps the Jobs' aggregated conditions, once per call. A source or
        federated object that is absent or being deleted is AllOK without an update (controller.go:270-284).
        Fetching the member objects and the Update call stay with the caller."""
        import time

        from . import statusagg as SA

        now = int(time.time()) if now is None else int(now)
        out: List[Optional[StatusAggOutcome]] = [None] * len(sources)
        batches = {SA.DEPLOYMENT: (SA.StatusAggBatch(SA.DEPLOYMENT), []), SA.JOB: (SA.StatusAggBatch(SA.JOB), [])}
        for i, (src, fed, objs) in enumerate(zip(sources, fed_objects, cluster_objs)):
            gone = lambda o: o is None or (o.get("metadata") or {}).get("deletionTimestamp") is not None  # noqa: E731
            if gone(src) or gone(fed):
                out[i] = StatusAggOutcome(STATUS_ALL_OK, False, None)
                continue
            kind = {"Deployment": SA.DEPLOYMENT, "Job": SA.JOB}.get(src.get("kind"))
            if kind is None:
                raise ValueError(f"reconcile_status_aggregation: no plugin for kind {src.get('kind')!r}")
            batches[kind][0].add(src, fed, objs)
            batches[kind][1].append(i)
        for batch, index in batches.values():
            if not index:
                continue
            arrays = batch.arrays()
            r = self.ctx.status_aggregate(**arrays) if batch.device else None
            for i, (need, err) in zip(index, batch.apply(r, now)):
                out[i] = StatusAggOutcome(STATUS_ERROR if err else STATUS_ALL_OK, need, str(err) if err else None)
        return out  # type: ignore[return-value]

    # ------------------------------------------------------------------ rollout planning
    def reconcile_rollout(self, objs: Sequence[dict], member_objs: Sequence[Dict[str, Optional[dict]]],
                          selected: Sequence, controller_order: Sequence[str] = ()) -> list:
        """The managed dispatcher's rollout planning for a batch of federated objects
        (pkg/controllers/sync/dispatch/managed.go:203-250): ``objs[i]`` is a federated Deployment,
        ``member_objs[i]`` its copy (or None) in every ready member cluster it could be fetched from and
        ``selected[i]`` the clusters its placement selects. One kad_rollout_plan answers every object
        (rollout.RolloutBatch); returns per object a rollout.RolloutOutcome with the plans, the overrides
        (GetRolloutOverrides), the dispatch action of every cluster and the status, or None for an object the
        planner does not see: the type config's RolloutPlan is not enabled, or spec.retainReplicas is true. A host
        error (an unsupported kind, replicas or annotations missing) makes the object ST_ERROR: its existing
        member objects are patched with their template kept. Dispatching stays with the caller."""
        from . import rollout as RO

        out: list = [None] * len(objs)
        if not getattr(self.type_config, "rollout_plan", False):
            return out
        batch, index = RO.RolloutBatch(self.type_config, controller_order), []
        for i, (fed, members, sel) in enumerate(zip(objs, member_objs, selected)):
            try:
                if RO.check_retain_replicas(fed):
                    continue
            except RO.RolloutError:  # CheckRetainReplicasFailed: Dispatch returns without dispatching
                continue
            batch.add(fed, members, sel)
            index.append(i)
        if index:
            for i, o in zip(index, batch.apply(self.ctx.rollout_plan(**batch.arrays()))):
                out[i] = o
        return out

    # ------------------------------------------------------------------ sync dispatch planning
    def reconcile_dispatch(self, objs: Sequence[dict], fed_namespaces: Optional[Dict[str, dict]], clusters: Sequence[dict],
                           member_objs: Sequence[Dict[str, object]], finalizer: Optional[str] = None,
                           limited_scope: bool = False) -> list:
        """The sync controller's cluster loop for a batch of federated objects (syncToClusters,
        pkg/controllers/sync/controller.go:425-544): ``objs[i]`` is a federated object, ``fed_namespaces`` the
        federated namespace objects by namespace name (None: none), ``clusters`` the joined FederatedCluster objects
        as dicts (conditions, deletion timestamp, annotations and finalizers are read) and ``member_objs[i]`` per
        cluster name the informer's member object, None where it holds none, or the exception its lookup failed
        with. ``finalizer``: the controller's cascading-delete finalizer (default: the one of the type config named
        ``<plural>.<group>``). One kad_dispatch_plan answers every object (dispatch.DispatchBatch); returns per
        object a dispatch.DispatchOutcome: the computed placement, the operation started and the propagation status
        recorded per cluster, whether to recheck after dispatch, ComputePlacementFailed. Its ``selected`` and
        ``rollout_members`` are what :meth:`reconcile_rollout` accepts. :meth:`reconcile_sync_versions` (before the
        operations) and :meth:`reconcile_sync_finish` (after them) are the rest of syncToClusters; objects being
        deleted (ensureDeletion) go to :meth:`reconcile_deletion` and the operations themselves are the caller's."""
        from . import dispatch as DI

        if finalizer is None:
            ftc = self.type_config
            finalizer = DI.cascading_delete_finalizer(ftc.plural_name + ("." + ftc.group if ftc.group else ""))
        batch = DI.DispatchBatch(self.type_config, clusters, finalizer, fed_namespaces, limited_scope)
        for fed, members in zip(objs, member_objs):
            batch.add(fed, members)
        if not len(batch):
            return []
        return batch.apply(self.ctx.dispatch_plan(**batch.arrays()))

    # ------------------------------------------------------------------ sync deletion
    def _deletion_batch(self, objs, clusters, member_objs, finalizer):
        from . import deletion as DL
        from . import dispatch as DI

        if finalizer is None:
            ftc = self.type_config
            finalizer = DI.cascading_delete_finalizer(ftc.plural_name + ("." + ftc.group if ftc.group else ""))
        batch = DL.DeletionBatch(self.type_config, clusters, finalizer)
        for fed, members in zip(objs, member_objs):
            batch.add(fed, members)
        return batch

    def reconcile_deletion(self, objs: Sequence[Optional[dict]], clusters: Sequence[dict],
                           member_objs: Sequence[Dict[str, object]], finalizer: Optional[str] = None) -> list:
        """The deletion arm of the sync controller's reconcile for a batch (ensureDeletion, deleteFromClusters,
        removeManagedLabel, handleDeletionInClusters: pkg/controllers/sync/controller.go:340-378, 723-979), before
        anything is sent: ``objs[i]`` is a federated object with a deletion timestamp (the ones
        :meth:`reconcile_dispatch`'s callers leave out), or None for a target without a federated object;
        ``clusters`` and ``member_objs[i]`` as :meth:`reconcile_dispatch` takes them. One kad_deletion_plan answers
        every object; returns per object a deletion.DeletionPlan: the delete and label-removal operations by cluster,
        the remaining clusters, the names the error texts list and the actions that come first."""
        batch = self._deletion_batch(objs, clusters, member_objs, finalizer)
        if not len(batch):
            return []
        return batch.apply_plan(self.ctx.deletion_plan(**batch.arrays()))

    def reconcile_deletion_finish(self, objs: Sequence[Optional[dict]], clusters: Sequence[dict],
                                  member_objs: Sequence[Dict[str, object]], op_results: Sequence[Dict[str, bool]],
                                  waits: Optional[Sequence[int]] = None, checks: Optional[Sequence[Dict[str, object]]] = None,
                                  check_clusters: Optional[Sequence[dict]] = None, finalizer: Optional[str] = None,
                                  plans: Optional[Sequence] = None) -> list:
        """What follows the operations of :meth:`reconcile_deletion` on the same batch: ``op_results[i]`` per cluster
        whether the operation succeeded, ``waits[i]`` the deletion.WAIT_* bits of the two Wait() calls, ``checks[i]``
        per cluster what ensureRemovedOrUnmanaged's GET answered other than NotFound (the member object, or the
        exception it failed with) and ``check_clusters`` the joined clusters as listed for the checks (default:
        unchanged). ``plans``: what :meth:`reconcile_deletion` returned for the same batch (the names the error texts
        list; default: restated on the host, without a second device call). One kad_deletion_finish decides every
        object; returns per object a deletion.DeletionOutcome: the worker result, the reason, the reference's error
        text and the actions that follow. DeleteVersions,
        deleteHistory, the finalizer's removal and RecordError stay with the caller."""
        batch = self._deletion_batch(objs, clusters, member_objs, finalizer)
        if not len(batch):
            return []
        if plans is None:
            from . import deletion as DL

            plans = batch.apply_plan(DL.plan_numpy(**batch.arrays()))
        res = self.ctx.deletion_finish(**batch.finish_arrays(op_results, waits, checks, check_clusters))
        return batch.apply_finish(res, plans, check_clusters)

    # ------------------------------------------------------------------ sync completion
    def reconcile_sync_versions(self, objs: Sequence[dict], outcomes: Sequence, desired: Sequence[Dict[str, dict]],
                                clusters: Sequence[str], versions, template_versions: Sequence[str],
                                override_versions: Sequence[str]) -> List[Dict[str, Tuple[bool, str]]]:
        """The version check of every update a :meth:`reconcile_dispatch` result starts (dispatch/managed.go:450-460:
        VersionForCluster, then util.ObjectNeedsUpdate, util/propagatedversion.go:54-119), between the dispatch
        plan and the operations: ``outcomes[i]`` is ``objs[i]``'s dispatch.DispatchOutcome, ``desired[i]`` per
        cluster the object the update would write (overrides applied, fields retained), ``clusters`` the joined
        cluster names, ``versions`` the syncfin.PropagatedVersions store and ``template_versions[i]`` /
        ``override_versions[i]`` the object's two hashes. One kad_sync_needs_update answers every (object, cluster)
        whose operation is an update; returns per object cluster → (the member object needs the update, the
        recorded version): where it needs none the caller records that version (managed.go:455-460)."""
        from . import dispatch as DI
        from . import syncfin as SF

        batch = SF.SyncFinishBatch(clusters)
        for fed, oc, want, tv, ov in zip(objs, outcomes, desired, template_versions, override_versions):
            md = fed.get("metadata") or {}
            k = batch.add_versions(versions.status(md.get("namespace", ""), md.get("name", "")), tv, ov)
            for name, op in sorted(oc.ops.items()):
                if op == DI.OP_UPDATE:
                    batch.add_update(k, name, want[name], oc.rollout_members[name], self.type_config.replicas_spec)
        if not batch.rows:
            return [{} for _ in objs]
        a = batch.needs_update_arrays()
        return batch.apply_needs_update(self.ctx.sync_needs_update(a.pop("n_clusters"), **a))

    def reconcile_sync_finish(self, objs: Sequence[dict], outcomes: Sequence, op_results: Sequence[Dict[str, dict]],
                              clusters: Sequence[str], versions, template_versions: Sequence[str],
                              override_versions: Sequence[str], collision_counts: Optional[Sequence[Optional[int]]] = None,
                              namespace_not_federated: Optional[Sequence[bool]] = None, now: Optional[str] = None) -> list:
        """The close of syncToClusters for a batch of federated objects whose Wait() did not time out
        (sync/controller.go:546-596): ``outcomes[i]`` is ``objs[i]``'s dispatch.DispatchOutcome and
        ``op_results[i]`` per cluster what its operation left: ``{"status": the propagation status it recorded on
        failure (absent: it succeeded, the timed-out status of the plan stands), "version": the version
        recordVersion recorded (absent: none), "updated": the member object was written}``. One kad_sync_finish
        decides Wait's transitions, the new cluster versions, status.clusters, the propagation condition and both
        writes (syncfin.SyncFinishBatch). The PropagatedVersion status is put into ``versions`` where it is to be
        written and ``objs[i]["status"]`` is replaced where UpdateStatus is due; ``now`` (RFC 3339, default the
        clock) stamps the condition. Returns per object a syncfin.FinishOutcome. The API writes stay with the
        caller."""
        import time

        from . import syncfin as SF

        now = time.strftime("%Y-%m-%dT%H:%M:%SZ", time.gmtime()) if now is None else now
        batch = SF.SyncFinishBatch(clusters)
        for i, (fed, oc, ops, tv, ov) in enumerate(zip(objs, outcomes, op_results, template_versions, override_versions)):
            md = fed.get("metadata") or {}
            records = {n: (ops.get(n, {}).get("status") or s, ops.get(n, {}).get("version") or "") for n, s in oc.status.items()}
            for n, r in ops.items():  # an operation on a cluster the plan gave no status
                records.setdefault(n, (r.get("status") or "", r.get("version") or ""))
            gen = md.get("generation", 0)
            batch.add(fed.get("status"), gen if isinstance(gen, int) else 0, collision_counts[i] if collision_counts else None,
                      oc.selected, records, any(r.get("updated") for r in ops.values()),
                      versions.status(md.get("namespace", ""), md.get("name", "")), tv, ov, oc.reason or SF.AGGREGATE_SUCCESS,
                      bool(namespace_not_federated[i]) if namespace_not_federated else False)
        if not len(batch):
            return []
        a = batch.finish_arrays()
        head = [a.pop(k) for k in ("n_clusters", "n_reasons", "reason_check_clusters", "reason_ns_not_federated")]
        out = batch.apply(self.ctx.sync_finish(*head, **a), now)
        for fed, o in zip(objs, out):
            md = fed.get("metadata") or {}
            if o.version_write:
                versions.set_status(md.get("namespace", ""), md.get("name", ""), o.version_status)
            if o.status_write:
                fed["status"] = o.status
        return out

    # ------------------------------------------------------------------ revision history
    def reconcile_revisions(self, objs: Sequence[dict], revisions: Sequence[Sequence[dict]],
                            pod_template_hashes: Optional[Sequence[Optional[str]]] = None) -> list:
        """The sync controller's syncRevisions for a batch of federated objects (pkg/controllers/sync/history.go:36-120,
        called at sync/controller.go:401-409 for a type with revisionHistoryEnabled): ``revisions[i]`` are the
        ControllerRevisions listed for ``objs[i]`` (history.list_revisions over the informer's store), in list order;
        ``pod_template_hashes[i]`` the object's getPodTemplateHash, appended to lastRevisionNameWithHash behind a ``|``
        where given (its go-spew hashing is the caller's). One kad_revision_plan hashes every patch, compares it with
        every listed revision's data and plans the creates, deletes, renumbers and relabels (history.RevisionBatch).
        Returns per object a history.RevisionOutcome: the ordered actions and syncRevisions' three return values, of
        which ``current_revision_name`` and ``last_revision_name_with_hash`` are what ensureAnnotations writes; a type
        without revisionHistoryEnabled gets empty outcomes. The API calls, the create-collision retry and the
        annotations' write stay with the caller."""
        from . import history as H

        if not self.type_config.revision_history:
            return [H.RevisionOutcome() for _ in objs]
        batch = H.batch_of(objs, revisions, pod_template_hashes)
        if not len(batch):
            return []
        return batch.apply(self.ctx.revision_plan(**batch.arrays()))

    # ------------------------------------------------------------------ policy reference counts
    def reconcile_policy_refcounts(self, events: Sequence[Tuple[object, Optional[dict]]], policies: Dict[tuple, dict],
                                   enqueued: Sequence[tuple] = ()) -> Tuple[list, list]:
        """The policy reference counter for a batch of federated-object events (pkg/controllers/policyrc:
        reconcileCount, controller.go:231-278, Counter.Update, counter.go:50-80, reconcilePersist,
        controller.go:280-366): ``events[i]`` is (the object's qualified name, the federated object as the informer
        holds it now, or None once it is deleted), in order; ``policies`` the propagation and override policy
        objects in the store by policyrc key ``(kind, namespace, name)``; ``enqueued`` the keys a policy informer
        event asks to persist. The counts live on this reconciler between calls (policyrc.PolicyRefCounter). One
        kad_policyrc_count answers every policy; the policies whose numbers moved get ``status.typedRefCount`` and
        ``status.refCount`` written in place. Returns (the flagged policy keys, the (key, policy) pairs to
        ``UpdateStatus``); raises policyrc.PolicyRefCountError where the reference panics. The informers and the
        ``UpdateStatus`` call with its conflict retry stay with the caller."""
        from . import policyrc as PR

        if self.policy_refs is None:
            self.policy_refs = PR.PolicyRefCounter(self.type_config)
        self.policy_refs.observe(events)
        arrays = self.policy_refs.arrays(policies, enqueued)
        result = self.ctx.policyrc_count(**arrays) if len(arrays["pol_flags"]) else None
        return self.policy_refs.apply(result, policies)

    # ------------------------------------------------------------------ monitor
    def reconcile_monitor(self, objs: Sequence[Tuple[str, Optional[dict]]], status_objs, member_objs, now: int,
                          status_enabled: bool = True,
                          kind: Optional[str] = None) -> Tuple[list, List[dict]]:
        """The monitor sub-controller for a batch of events (pkg/controllers/monitor, MonitorSubController.reconcile,
        monitor_subcontroller.go:172-343): ``objs[i]`` is (the object's qualified name, the federated object as the
        informer holds it now, or None), in order; ``status_objs`` / ``member_objs`` the status object and the
        (cluster name, member object) pairs, either as dicts by qualified name (what the stores hold now) or as
        sequences aligned with ``objs`` (what each event saw: two events of one key may differ, and the per-key
        split runs them in order); ``now`` in ns since the Unix epoch; ``kind`` the
        federated kind (default ``Federated<Kind>``). The meters live on this reconciler's context between calls
        (monitor.MeterTable beside the device table). Returns (one monitor.MonitorOutcome per event, copies of the
        objects whose ``lastGeneration`` annotation is to be written, annotated). The Update call stays with the
        caller."""
        from . import monitor as M

        if self.meters is None:
            self.meters = M.MeterTable()
        kind = kind or "Federated" + self.type_config.kind

        def of(src, i, name, default):
            return src.get(name, default) if isinstance(src, dict) else src[i]

        events = [dict(key=f"{kind}/{name}", obj=obj, status_enabled=status_enabled, status=of(status_objs, i, name, None),
                       members=of(member_objs, i, name, ())) for i, (name, obj) in enumerate(objs)]

        def reserve(need: int) -> None:
            if need > self.ctx.monitor_info()["capacity"]:
                self.ctx.monitor_reserve(max(1024, 1 << (need - 1).bit_length()))

        outcomes = self.meters.reconcile(events, now, self.ctx.monitor_reconcile, reserve)
        updates = []
        for (_, obj), o in zip(objs, outcomes):
            if o.update_annotation:
                meta = dict(obj.get("metadata", {}))
                meta["annotations"] = {**(meta.get("annotations") or {}), "lastGeneration": o.last_generation}
                updates.append({**obj, "metadata": meta})
        return outcomes, updates

    def monitor_report(self, now: int) -> List[tuple]:
        """DoReport (report.go:31-163) at ``now`` over every meter: one kad_monitor_report; the metrics as
        monitor.Report.to_metrics gives them."""
        from . import monitor as M

        if self.meters is None:
            self.meters = M.MeterTable()
        return M.Report.from_result(self.meters, self.ctx.monitor_report(now, self.meters.n_types)).to_metrics()

    # ------------------------------------------------------------------ the reconcile over JSON texts
    def reconcile_texts(self, texts: Sequence, policies: Sequence, clusters: List[T.FederatedCluster],
                        profiles: Optional[Dict[str, Optional[dict]]] = None
                        ) -> Tuple[List[ReconcileOutcome], List[Optional[bytes]]]:
        """:meth:`reconcile` over the federated objects' JSON texts (what an informer or a watch hands over),
        with every per-object step native: the trigger JSON's object part (kad_trigger_prefixes), the trigger
        hashes (kad_trigger_run), the SchedulingUnits (kad_units_from_objects), the schedule (kad_schedule) and
        the write-back with the trigger annotation (kad_apply_results). ``policies``: the
        (Cluster)PropagationPolicies' JSON; each object's policy is found through its labels as
        MatchedPolicyKey does. Returns the outcomes (stages as :meth:`reconcile`, plus ``bad-json`` and
        ``policy-error`` for texts that do not decode) and per object its new text — the deep copy the
        reference goes on to Update (``scheduled``) or holds when it skips scheduling (``no-scheduling``) —
        or None where the reconcile left the object as it was or dropped its copy on an error."""
        import json

        from . import columns as K
        from .results import to_schedule_result_cols

        profiles = profiles or {}
        self._pass = None
        ot, pt = K._texts(texts), K._texts(policies)
        n = len(ot)
        out: List[Optional[ReconcileOutcome]] = [None] * n
        new_text: List[Optional[bytes]] = [None] * n
        pols: List[Optional[O.PropagationPolicy]] = []
        for t in pt:  # a handful: decoded once for the profile name and the apply parameters
            try:
                pols.append(O.PropagationPolicy.from_json(json.loads(t)))
            except Exception:  # noqa: BLE001 — the native lookup reports it as KAD_OBJ_POLICY_ERROR
                pols.append(None)
        tr = K.trigger_prefixes(self.type_config, ot, pt)

        # prepareToSchedule :349-392 — policy and profile lookup, then the trigger JSON (:394-399)
        hashed: List[int] = []
        pol_of = tr.policy_index
        for i in range(n):
            st = int(tr.status[i])
            if st == K.OBJ_POLICY_NOT_FOUND:
                out[i] = ReconcileOutcome(STATUS_ALL_OK, "policy-not-found")
                continue
            if st == K.OBJ_BAD_JSON:
                out[i] = ReconcileOutcome(STATUS_ERROR, "bad-json", error=tr.messages[i])
                continue
            if st == K.OBJ_POLICY_ERROR:
                out[i] = ReconcileOutcome(STATUS_ERROR, "policy-error", error=tr.messages[i])
                continue
            p = pols[pol_of[i]] if pol_of[i] >= 0 else None
            if p is None and pol_of[i] >= 0:  # the library decoded it but objects.py did not: not scheduled on
                out[i] = ReconcileOutcome(STATUS_ERROR, "policy-error", error="policy does not decode")
                continue
            if p is not None and p.spec.scheduling_profile and p.spec.scheduling_profile not in profiles:
                out[i] = ReconcileOutcome(STATUS_ALL_OK, "profile-not-found")
                continue
            if st != K.OBJ_OK:
                out[i] = ReconcileOutcome(STATUS_ERROR, "trigger-error", error=tr.messages[i])
                continue
            hashed.append(i)

        # :394-421 — the hashes in one GPU pass; AddAnnotation's "changed" against the current annotation
        key = T.clusters_fingerprint(clusters)
        if key != self._clusters_key:
            self.hasher.set_clusters(clusters)
            self._clusters_key = key
        self.ctx.trigger_prefixes_upload([tr.prefixes[i] for i in hashed])
        self.ctx.trigger_run()
        hashes = self.ctx.trigger_download()
        trig: List[Optional[str]] = [None] * n
        ann_only = [False] * n
        to_schedule: List[int] = []
        for i, h in zip(hashed, hashes.tolist()):
            hv = O.format_trigger_hash(h)
            if tr.flags[i] & K.TRIG_HAS_HASH and tr.current_hash[i] == hv:
                out[i] = ReconcileOutcome(STATUS_ALL_OK, "unchanged")
                continue
            trig[i] = hv
            if tr.flags[i] & K.TRIG_NO_SCHEDULING:
                out[i] = ReconcileOutcome(STATUS_ALL_OK, "no-scheduling")
                ann_only[i] = True
            else:
                to_schedule.append(i)

        # schedule :445-521 — per framework one native unit build and one GPU batch
        results: Dict[int, T.ScheduleResult] = {}
        groups: Dict[Optional[str], List[int]] = {}
        for i in to_schedule:
            p = pols[pol_of[i]] if pol_of[i] >= 0 else None
            if p is None:
                results[i] = T.ScheduleResult({})  # :454-467 no policy: schedule to no clusters
                continue
            groups.setdefault(p.spec.scheduling_profile or None, []).append(i)
        # the unit is built from the object after AddAnnotation (:407); that only differs where the annotation
        # replaced annotations that were not a string map (the typed view would reject the old ones)
        unit_text = {}
        fix = [i for i in to_schedule if tr.flags[i] & K.TRIG_ANN_NOT_MAP]
        if fix:
            a = K.apply_results_ex(self.type_config, [ot[i] for i in fix], [], [0] * (len(fix) + 1), [], [],
                                   trigger=[trig[i] for i in fix], ann_only=[True] * len(fix))
            unit_text = {i: a.texts[k] for k, i in enumerate(fix) if a.status[k] == K.APPLY_OK}
        names: List[str] = []
        for prof_name, members in groups.items():
            try:
                fwk = self._framework(profiles.get(prof_name) if prof_name else None)
            except F.FrameworkError as e:
                for i in members:
                    out[i] = ReconcileOutcome(STATUS_ERROR, "framework-error", error=str(e))
                continue
            built = K.units_from_objects(self.type_config, [unit_text.get(i, ot[i]) for i in members], pt,
                                         [int(pol_of[i]) for i in members])
            ok = []
            for k, i in enumerate(members):
                if built.status[k] == K.OBJ_OK:
                    ok.append((i, int(built.unit_index[k])))
                else:
                    out[i] = ReconcileOutcome(STATUS_ERROR, "unit-error", error=built.messages[k])
            if not ok:
                continue
            res, snap = self.scheduler.schedule_columns(fwk, built.cols, clusters)
            names = snap.names
            self._record_pass(len(res.status), ok, out)
            for i, w in ok:
                r = to_schedule_result_cols(res, w, built.cols, names)
                if isinstance(r, T.ScheduleError):
                    out[i] = ReconcileOutcome(STATUS_ERROR, "schedule-error", error=str(r))
                else:
                    results[i] = r

        # reconcile :291-308 + applySchedulingResult, and the no-scheduling objects' annotation, in one pass
        todo, follower, threshold = [], [], []
        params: Dict[int, object] = {}  # per policy: (follower, threshold) or the error
        for i in range(n):
            if ann_only[i]:
                todo.append(i)
                follower.append(False)
                threshold.append(None)
            elif i in results:
                pi = int(pol_of[i])
                if pi not in params:
                    try:
                        params[pi] = self._apply_params(pols[pi] if pi >= 0 else None)
                    except (O.ObjectError, O.GoPanic) as e:
                        params[pi] = e
                ft = params[pi]
                if isinstance(ft, Exception):
                    out[i] = ReconcileOutcome(STATUS_ERROR, "apply-error", result=results[i], error=str(ft))
                    continue
                f, t = ft
                todo.append(i)
                follower.append(f)
                threshold.append(t)
        if not todo:
            return out, new_text  # type: ignore[return-value]
        table = list(names)
        at = {c: k for k, c in enumerate(table)}
        off, cl, rep = [0], [], []
        for i in todo:
            if not ann_only[i]:
                for c, v in (results[i].suggested_clusters or {}).items():
                    if c not in at:  # a sticky result's cluster that left the snapshot
                        at[c] = len(table)
                        table.append(c)
                    cl.append(at[c])
                    rep.append(-1 if v is None else v)
            off.append(len(cl))
        a = K.apply_results_ex(self.type_config, [ot[i] for i in todo], table, off, cl, rep, follower, threshold,
                               trigger=[trig[i] for i in todo], ann_only=[ann_only[i] for i in todo],
                               with_fields=False)
        for k, i in enumerate(todo):
            if a.status[k] != K.APPLY_OK:
                out[i] = ReconcileOutcome(STATUS_ERROR, "apply-error", result=results.get(i), error=a.messages[k])
                continue
            if a.changed[k]:
                new_text[i] = a.texts[k]
            if not ann_only[i]:
                out[i] = ReconcileOutcome(STATUS_ALL_OK, "scheduled", True, bool(a.modified[k]), results[i])
        return out, new_text  # type: ignore[return-value]
