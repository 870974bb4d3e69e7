"""ctypes binding of libkad.so and the ScheduleAlgorithm-shaped host API.

``BatchScheduler.schedule(fwk, units, clusters)`` is the batch counterpart of
``core.ScheduleAlgorithm.Schedule(ctx, fwk, su, clusters)``
(pkg/controllers/scheduler/core/generic_scheduler.go:37-44): same inputs (a
framework, scheduling units, the cluster list), same per-unit output
(``ScheduleResult`` or the error class). There is no CPU fallback: if the HIP
library or a GPU is missing this raises.
"""

from __future__ import annotations

import ctypes
import os
import re
from typing import List, Optional, Sequence, Union

import numpy as np

from . import types as T
from .framework import Framework
from . import pack as _pack
from .pack import Batch, Snapshot, SnapshotDelta
from .results import BatchResult, FilterDiagnosis, to_schedule_result

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, "libkad.so")
HEADER = os.path.join(os.path.dirname(HERE), "include", "kad_sched.h")

KAD_ERRORS = {-1: "KAD_EINVAL", -2: "KAD_EHIP", -3: "KAD_ENOMEM", -4: "KAD_ESTATE", -5: "KAD_EUNSUPPORTED",
              -6: "KAD_EHOST", -7: "KAD_ENOSPC"}
KAD_EINVAL, KAD_ESTATE, KAD_EUNSUPPORTED, KAD_ENOSPC = -1, -4, -5, -7


class KadError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"{KAD_ERRORS.get(code, code)}: {msg}")
        self.code = code


class ResultView(ctypes.Structure):
    _fields_ = [("status", ctypes.c_void_p), ("count", ctypes.c_void_p), ("flags", ctypes.c_void_p),
                ("cluster", ctypes.c_void_p), ("replicas", ctypes.c_void_p)]


class ExplainView(ctypes.Structure):  # kad_explain_view
    _fields_ = [("rejected", ctypes.c_void_p), ("feasible", ctypes.c_void_p), ("fit_detail", ctypes.c_void_p),
                ("first_fail", ctypes.c_void_p)]


class ResultState(ctypes.Structure):  # kad_result_state
    _fields_ = [("n_units", ctypes.c_int32), ("place_off", ctypes.c_void_p), ("place_cluster", ctypes.c_void_p),
                ("place_has", ctypes.c_void_p), ("ovr_off", ctypes.c_void_p), ("ovr_cluster", ctypes.c_void_p),
                ("ovr_value", ctypes.c_void_p), ("ovr_kind", ctypes.c_void_p)]


class OverrideBatch(ctypes.Structure):  # kad_override_batch
    _fields_ = [("n_objects", ctypes.c_int32), ("rule_words", ctypes.c_int32), ("obj_policy", ctypes.c_void_p),
                ("place_off", ctypes.c_void_p), ("place_cluster", ctypes.c_void_p)]


class OverrideView(ctypes.Structure):  # kad_override_view
    _fields_ = [("status", ctypes.c_void_p), ("matched", ctypes.c_void_p)]


class FollowerBatch(ctypes.Structure):  # kad_follower_batch
    _fields_ = [("n_ids", ctypes.c_int32), ("n_leaders", ctypes.c_int32), ("n_followers", ctypes.c_int32),
                ("flags", ctypes.c_uint32), ("lead_off", ctypes.c_void_p), ("lead_cluster", ctypes.c_void_p),
                ("sched_off", ctypes.c_void_p), ("sched_cluster", ctypes.c_void_p), ("keep_off", ctypes.c_void_p),
                ("keep_cluster", ctypes.c_void_p), ("fol_off", ctypes.c_void_p), ("fol_leader", ctypes.c_void_p),
                ("cur_off", ctypes.c_void_p), ("cur_cluster", ctypes.c_void_p), ("cur_has", ctypes.c_void_p),
                ("out_capacity", ctypes.c_int64)]


class FollowerView(ctypes.Structure):  # kad_follower_view
    _fields_ = [("changed", ctypes.c_void_p), ("count", ctypes.c_void_p), ("out_off", ctypes.c_void_p),
                ("out_cluster", ctypes.c_void_p)]


class MigrateBatch(ctypes.Structure):  # kad_migrate_batch
    _fields_ = [("n_ids", ctypes.c_int32), ("n_objects", ctypes.c_int32), ("n_segments", ctypes.c_int32),
                ("n_old", ctypes.c_int32), ("n_pods", ctypes.c_int64), ("now_ns", ctypes.c_int64),
                ("obj_seg_off", ctypes.c_void_p), ("obj_threshold_ns", ctypes.c_void_p), ("seg_cluster", ctypes.c_void_p),
                ("seg_desired", ctypes.c_void_p), ("seg_flags", ctypes.c_void_p), ("seg_pod_off", ctypes.c_void_p),
                ("pod_t_ns", ctypes.c_void_p), ("pod_flags", ctypes.c_void_p), ("old_off", ctypes.c_void_p),
                ("old_cluster", ctypes.c_void_p), ("old_cap", ctypes.c_void_p)]


class MigrateView(ctypes.Structure):  # kad_migrate_view
    _fields_ = [("uns", ctypes.c_void_p), ("next_cross", ctypes.c_void_p), ("cap", ctypes.c_void_p),
                ("changed", ctypes.c_void_p), ("n_written", ctypes.c_void_p), ("retry_after", ctypes.c_void_p),
                ("backoff", ctypes.c_void_p)]


class CstatBatch(ctypes.Structure):  # kad_cstat_batch
    _fields_ = [("n_clusters", ctypes.c_int32), ("n_res", ctypes.c_int32), ("n_nodes", ctypes.c_int64),
                ("n_pods", ctypes.c_int64), ("n_node_ents", ctypes.c_int64), ("n_pod_ents", ctypes.c_int64),
                ("cl_node_off", ctypes.c_void_p), ("node_flags", ctypes.c_void_p), ("node_ent_off", ctypes.c_void_p),
                ("nent_res", ctypes.c_void_p), ("nent_val", ctypes.c_void_p), ("cl_pod_off", ctypes.c_void_p),
                ("pod_flags", ctypes.c_void_p), ("pod_ent_off", ctypes.c_void_p), ("pent_res", ctypes.c_void_p),
                ("pent_kind", ctypes.c_void_p), ("pent_val", ctypes.c_void_p)]


class CstatView(ctypes.Structure):  # kad_cstat_view
    _fields_ = [("alloc", ctypes.c_void_p), ("avail", ctypes.c_void_p), ("has", ctypes.c_void_p),
                ("sched_nodes", ctypes.c_void_p)]


class SaggBatch(ctypes.Structure):  # kad_sagg_batch
    _fields_ = [("kind", ctypes.c_int32), ("n_objects", ctypes.c_int32), ("n_segments", ctypes.c_int32),
                ("reserved", ctypes.c_int32), ("obj_seg_off", ctypes.c_void_p), ("obj_flags", ctypes.c_void_p),
                ("obj_generation", ctypes.c_void_p), ("obj_observed", ctypes.c_void_p), ("old_vals", ctypes.c_void_p),
                ("seg_vals", ctypes.c_void_p), ("seg_flags", ctypes.c_void_p), ("seg_observed", ctypes.c_void_p),
                ("seg_synced", ctypes.c_void_p), ("seg_start", ctypes.c_void_p), ("seg_done", ctypes.c_void_p)]


class SaggView(ctypes.Structure):  # kad_sagg_view
    _fields_ = [("sums", ctypes.c_void_p), ("changed", ctypes.c_void_p), ("observed", ctypes.c_void_p),
                ("start_min", ctypes.c_void_p), ("done_max", ctypes.c_void_p), ("n_done", ctypes.c_void_p),
                ("n_failed", ctypes.c_void_p), ("finished", ctypes.c_void_p)]


class RolloutBatch(ctypes.Structure):  # kad_rollout_batch
    _fields_ = [("n_objects", ctypes.c_int32), ("n_targets", ctypes.c_int32), ("obj_tgt_off", ctypes.c_void_p),
                ("obj_max_surge", ctypes.c_void_p), ("obj_max_unavailable", ctypes.c_void_p),
                ("obj_replicas", ctypes.c_void_p), ("obj_flags", ctypes.c_void_p), ("tgt_vals", ctypes.c_void_p),
                ("tgt_flags", ctypes.c_void_p)]


class RolloutView(ctypes.Structure):  # kad_rollout_view
    _fields_ = [("replicas", ctypes.c_void_p), ("max_surge", ctypes.c_void_p), ("max_unavailable", ctypes.c_void_p),
                ("plan_flags", ctypes.c_void_p), ("action", ctypes.c_void_p), ("status", ctypes.c_void_p)]


class DispatchBatch(ctypes.Structure):  # kad_dispatch_batch
    _fields_ = [("n_clusters", ctypes.c_int32), ("n_objects", ctypes.c_int32), ("n_namespaces", ctypes.c_int32),
                ("cluster_flags", ctypes.c_void_p), ("obj_flags", ctypes.c_void_p), ("obj_ns", ctypes.c_void_p),
                ("obj_pl_off", ctypes.c_void_p), ("pl_cluster", ctypes.c_void_p), ("ns_pl_off", ctypes.c_void_p),
                ("ns_cluster", ctypes.c_void_p), ("obj_ob_off", ctypes.c_void_p), ("ob_cluster", ctypes.c_void_p),
                ("ob_flags", ctypes.c_void_p), ("out_off", ctypes.c_void_p)]


class DispatchView(ctypes.Structure):  # kad_dispatch_view
    _fields_ = [("out_cluster", ctypes.c_void_p), ("out_op", ctypes.c_void_p), ("out_status", ctypes.c_void_p),
                ("count", ctypes.c_void_p), ("n_ops", ctypes.c_void_p), ("n_selected", ctypes.c_void_p),
                ("obj_result", ctypes.c_void_p)]


class PolicyrcBatch(ctypes.Structure):  # kad_policyrc_batch
    _fields_ = [("n_policies", ctypes.c_int32), ("n_dec", ctypes.c_int32), ("n_inc", ctypes.c_int32),
                ("reserved", ctypes.c_int32), ("dec_ids", ctypes.c_void_p), ("inc_ids", ctypes.c_void_p),
                ("count", ctypes.c_void_p), ("stored_typed", ctypes.c_void_p), ("stored_rest", ctypes.c_void_p),
                ("stored_total", ctypes.c_void_p), ("pol_flags", ctypes.c_void_p)]


class PolicyrcView(ctypes.Structure):  # kad_policyrc_view
    _fields_ = [("new_count", ctypes.c_void_p), ("new_total", ctypes.c_void_p), ("state", ctypes.c_void_p),
                ("n_negative", ctypes.c_void_p)]


class SyncNuBatch(ctypes.Structure):  # kad_sync_nu_batch
    _fields_ = [("n_clusters", ctypes.c_int32), ("n_objects", ctypes.c_int32), ("n_rows", ctypes.c_int32),
                ("n_versions", ctypes.c_int32), ("row_obj", ctypes.c_void_p), ("row_cluster", ctypes.c_void_p),
                ("row_target", ctypes.c_void_p), ("row_flags", ctypes.c_void_p), ("obj_flags", ctypes.c_void_p),
                ("rec_off", ctypes.c_void_p), ("rec_cluster", ctypes.c_void_p), ("rec_version", ctypes.c_void_p),
                ("ver_flags", ctypes.c_void_p)]


class SyncNuView(ctypes.Structure):  # kad_sync_nu_view
    _fields_ = [("needs_update", ctypes.c_void_p), ("recorded", ctypes.c_void_p)]


class SyncFinBatch(ctypes.Structure):  # kad_sync_fin_batch
    _fields_ = [("n_clusters", ctypes.c_int32), ("n_objects", ctypes.c_int32), ("n_versions", ctypes.c_int32),
                ("n_reasons", ctypes.c_int32), ("reason_check_clusters", ctypes.c_int32),
                ("reason_ns_not_federated", ctypes.c_int32), ("obj_flags", ctypes.c_void_p), ("reason_in", ctypes.c_void_p),
                ("cond_reason", ctypes.c_void_p), ("sel_off", ctypes.c_void_p), ("sel_cluster", ctypes.c_void_p),
                ("ent_off", ctypes.c_void_p), ("ent_cluster", ctypes.c_void_p), ("ent_status", ctypes.c_void_p),
                ("ent_version", ctypes.c_void_p), ("oldv_off", ctypes.c_void_p), ("oldv_cluster", ctypes.c_void_p),
                ("oldv_version", ctypes.c_void_p), ("olds_off", ctypes.c_void_p), ("olds_cluster", ctypes.c_void_p),
                ("olds_status", ctypes.c_void_p), ("olds_gen", ctypes.c_void_p), ("ver_gen", ctypes.c_void_p),
                ("ver_flags", ctypes.c_void_p), ("ver_off", ctypes.c_void_p), ("st_off", ctypes.c_void_p)]


class SyncFinView(ctypes.Structure):  # kad_sync_fin_view
    _fields_ = [("out_ver_cluster", ctypes.c_void_p), ("out_ver_id", ctypes.c_void_p), ("ver_count", ctypes.c_void_p),
                ("ver_write", ctypes.c_void_p), ("out_st_cluster", ctypes.c_void_p), ("out_st_status", ctypes.c_void_p),
                ("out_st_gen", ctypes.c_void_p), ("st_count", ctypes.c_void_p), ("obj_out", ctypes.c_void_p),
                ("reason_out", ctypes.c_void_p)]


class MonitorBatch(ctypes.Structure):  # kad_monitor_batch
    _fields_ = [("n_objects", ctypes.c_int32), ("n_clusters", ctypes.c_int32), ("now_ns", ctypes.c_int64),
                ("slot", ctypes.c_void_p), ("obj_flags", ctypes.c_void_p), ("type_id", ctypes.c_void_p),
                ("creation_ns", ctypes.c_void_p), ("sync_success_ns", ctypes.c_void_p), ("fed_off", ctypes.c_void_p),
                ("fed_cluster", ctypes.c_void_p), ("fed_gen", ctypes.c_void_p), ("mem_off", ctypes.c_void_p),
                ("mem_cluster", ctypes.c_void_p), ("mem_gen", ctypes.c_void_p), ("last_off", ctypes.c_void_p),
                ("last_cluster", ctypes.c_void_p), ("last_gen", ctypes.c_void_p)]


class MonitorView(ctypes.Structure):  # kad_monitor_view
    _fields_ = [("result", ctypes.c_void_p), ("bits", ctypes.c_void_p), ("meter", ctypes.c_void_p),
                ("would", ctypes.c_void_p)]


class RevisionBatch(ctypes.Structure):  # kad_revision_batch
    _fields_ = [("n_objects", ctypes.c_int32), ("n_pairs", ctypes.c_int32), ("blob_len", ctypes.c_int64),
                ("action_capacity", ctypes.c_int64), ("limit", ctypes.c_void_p), ("collision", ctypes.c_void_p),
                ("obj_flags", ctypes.c_void_p), ("patch_off", ctypes.c_void_p), ("patch_len", ctypes.c_void_p),
                ("blob", ctypes.c_void_p), ("rev_off", ctypes.c_void_p), ("rev_data_off", ctypes.c_void_p),
                ("rev_data_len", ctypes.c_void_p), ("rev_revision", ctypes.c_void_p), ("rev_time", ctypes.c_void_p),
                ("rev_name_rank", ctypes.c_void_p), ("rev_flags", ctypes.c_void_p), ("rev_hash", ctypes.c_void_p),
                ("rev_lab_off", ctypes.c_void_p), ("rev_lab", ctypes.c_void_p), ("want_off", ctypes.c_void_p),
                ("want_lab", ctypes.c_void_p)]


class RevisionView(ctypes.Structure):  # kad_revision_view
    _fields_ = [("out_off", ctypes.c_void_p), ("hash", ctypes.c_void_p), ("upd_hash", ctypes.c_void_p),
                ("upd_parsed", ctypes.c_void_p), ("equal", ctypes.c_void_p), ("order", ctypes.c_void_p),
                ("n_old", ctypes.c_void_p), ("keep", ctypes.c_void_p), ("n_actions", ctypes.c_void_p),
                ("last", ctypes.c_void_p), ("rev_number", ctypes.c_void_p), ("act_kind", ctypes.c_void_p),
                ("act_rev", ctypes.c_void_p)]


class DeletionBatch(ctypes.Structure):  # kad_deletion_batch
    _fields_ = [("n_clusters", ctypes.c_int32), ("n_objects", ctypes.c_int32), ("cluster_flags", ctypes.c_void_p),
                ("obj_flags", ctypes.c_void_p), ("obj_ob_off", ctypes.c_void_p), ("ob_cluster", ctypes.c_void_p),
                ("ob_flags", ctypes.c_void_p)]


class DeletionView(ctypes.Structure):  # kad_deletion_view
    _fields_ = [("out_op", ctypes.c_void_p), ("n_ops", ctypes.c_void_p), ("n_remaining", ctypes.c_void_p),
                ("n_retrieval_failed", ctypes.c_void_p), ("obj_pre", ctypes.c_void_p), ("obj_first", ctypes.c_void_p)]


class DeletionResults(ctypes.Structure):  # kad_deletion_results
    _fields_ = [("op_ok", ctypes.c_void_p), ("obj_wait", ctypes.c_void_p), ("chk_off", ctypes.c_void_p),
                ("chk_cluster", ctypes.c_void_p), ("chk_flags", ctypes.c_void_p), ("chk_cluster_flags", ctypes.c_void_p)]


class DeletionFinishView(ctypes.Structure):  # kad_deletion_finish_view
    _fields_ = [("obj_status", ctypes.c_void_p), ("obj_reason", ctypes.c_void_p), ("obj_then", ctypes.c_void_p),
                ("n_failed_ops", ctypes.c_void_p), ("n_failed_checks", ctypes.c_void_p)]


class MonitorReportBatch(ctypes.Structure):  # kad_monitor_report_batch
    _fields_ = [("now_ns", ctypes.c_int64), ("n_types", ctypes.c_int32), ("timer_cap", ctypes.c_int32)]


class MonitorReportView(ctypes.Structure):  # kad_monitor_report_view
    _fields_ = [("counters", ctypes.c_void_p), ("type_sync", ctypes.c_void_p), ("type_status", ctypes.c_void_p),
                ("sync_slot", ctypes.c_void_p), ("sync_ms", ctypes.c_void_p), ("status_slot", ctypes.c_void_p),
                ("status_ms", ctypes.c_void_p), ("n_timers", ctypes.c_void_p)]


_lib = None


def declared_functions() -> List[str]:
    """Names of the functions include/*.h declare (kad_sched.h, kad_pack.h, kad_objects.h)."""
    import glob

    names = set()
    for h in sorted(glob.glob(os.path.join(os.path.dirname(HEADER), "*.h"))):
        with open(h) as f:
            names |= set(re.findall(r"^\s*(?:int|void|const char\*)\s+(kad_\w+)\s*\(", f.read(), re.M))
    return sorted(names)


# kad_route_eval's records (include/kad_sched.h): the inputs with the defaults of the tuning fields, the outputs
ROUTE_IN = dict(C=0, clean=0, fold=0, fitfold=0, TW=1, snap_negative=0, W=1, has_current=0, zero_req=0, batch_defer=0,
                batch_many_terms=0, filter_mask=0, score_mask=0, debug_capture=0, side_stream=1, n_cu=256, no_rows=0,
                rows_after=0, rows_no_inline=0, prep_wave=1, wide_min_nch=5, lean_blocks_per_cu=0, rows16=0)
ROUTE_OUT = ("prep", "prep_lanes", "family", "variant", "row_variant", "full_variant", "use_rows", "early_rows",
             "may_defer", "rows", "defer_pass", "cache_ne", "cache_pn", "cache_zs", "wpb", "threads", "lds", "wave_bytes",
             "grid", "batch", "row_grid")
_ROUTE_ENUMS = {"prep": ("PREP", "PREP_WAVE2", "PREP_WAVE3", "PREP_WAVE4", "PREP_VEC"), "family": ("LEAN", "WIDE"),
                "rows": ("NONE", "INLINE", "BESIDE", "AFTER")}


def _route_dict(L, out) -> dict:
    d = dict(zip(ROUTE_OUT, out))
    for k in ("variant", "row_variant", "full_variant"):
        d[k] = L.kad_route_variant_name(d[k]).decode()
    for k, names in _ROUTE_ENUMS.items():
        d[k] = names[d[k]]
    return d


def route_eval(per_cu: int = 1, row_per_cu: int = 1, **inputs) -> dict:
    """kad_route_eval: the library's route decision on the given inputs (ROUTE_IN's fields; needs no GPU), with
    the kernel variants, the prep kernel, the family and the row placement as their enum names."""
    L = load_library()
    bad = set(inputs) - set(ROUTE_IN)
    if bad:
        raise TypeError(f"unknown route inputs {sorted(bad)}")
    rin = (ctypes.c_int32 * len(ROUTE_IN))(*[int(inputs.get(k, v)) for k, v in ROUTE_IN.items()])
    out = (ctypes.c_int32 * len(ROUTE_OUT))()
    rc = L.kad_route_eval(rin, per_cu, row_per_cu, out)
    if rc != 0:
        raise ValueError(f"kad_route_eval: {rc}")
    return _route_dict(L, out)


_I32, _I64 = ctypes.c_int32, ctypes.c_int64
# The consumer calls' ABI by call name: the call itself, then the arguments that follow (batch, view) in
# kad_<name>_check, the inputs of kad_<name>_route_eval, and those of kad_<name>_debug_route (None: it has none).
# kad_<name>_timing and kad_<name>_last_route take (ctx, out).
_CONSUMER_ABI = {
    "follower": ("kad_follower_union", (_I32, _I32), (_I32, _I32, _I32), None),
    "migrate": ("kad_migrate_estimate", (_I32,), (_I32, _I64, _I32, _I32, _I32), (_I32, _I32)),
    "cstat": ("kad_cluster_resources", (), (_I32, _I32, _I64, _I64, _I32, _I32), (_I32, _I32)),
    "sagg": ("kad_status_aggregate", (), (_I32, _I32, _I64, _I32), (_I32, _I32)),
    "rollout": ("kad_rollout_plan", (ctypes.c_void_p,), (_I32, _I32, _I64, _I32, _I32), (_I32, _I32, _I32)),
    "dispatch": ("kad_dispatch_plan", (), (_I32, _I32, _I32), None),
    "policyrc": ("kad_policyrc_count", (), (_I32, _I64, _I32), (_I32,)),
    "sync_needs_update": ("kad_sync_needs_update", (), (_I32, _I32), None),
    "sync_finish": ("kad_sync_finish", (), (_I32, _I32, _I64, _I32), (_I32, _I32)),
    "monitor_reconcile": ("kad_monitor_reconcile", (), (_I32, _I32, _I64, _I32), (_I32, _I32)),
    "monitor_report": ("kad_monitor_report", (), (_I64, _I32, _I32), (_I32, _I32)),
    "revision_plan": ("kad_revision_plan", (), (_I32, _I32, _I32, _I64, _I64, _I64, _I32), (_I32, _I32)),
    "deletion": ("kad_deletion_plan", (), (_I32, _I32, _I32, _I64, _I32), (_I32, _I32)),
    # (kad_deletion_finish itself takes the results between the batch and the view: bound below the loop)
    "deletion_finish": ("kad_deletion_finish", (ctypes.c_void_p,), (_I32, _I32, _I32, _I64, _I32), (_I32, _I32)),
}


def load_library(path: str = LIB_PATH):
    """Load libkad.so (fails loudly: the product path has no CPU fallback)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(path):
        raise RuntimeError(f"libkad.so not built at {path}: run `python -m kubeadmiral_amd.build`")
    L = ctypes.CDLL(path)
    P, I, U32, SZ = ctypes.c_void_p, ctypes.c_int, ctypes.c_uint32, ctypes.c_size_t
    L.kad_abi_version.restype = I
    L.kad_ctx_create.argtypes = [I, ctypes.POINTER(P)]
    L.kad_ctx_destroy.argtypes = [P]
    L.kad_last_error.argtypes = [P]
    L.kad_last_error.restype = ctypes.c_char_p
    L.kad_snapshot_upload.argtypes = [P, P, SZ]
    L.kad_snapshot_upload_device.argtypes = [P, P, SZ]
    L.kad_snapshot_update.argtypes = [P, P, SZ]
    L.kad_batch_upload.argtypes = [P, P, SZ]
    L.kad_schedule.argtypes = [P, P]
    L.kad_sync.argtypes = [P]
    L.kad_last_timing.argtypes = [P, P]
    L.kad_set_timing.argtypes = [P, I]
    L.kad_results_download.argtypes = [P, P]
    L.kad_results_copy_device.argtypes = [P, P]
    L.kad_stage_timing.argtypes = [P, P, I]
    L.kad_path_counts.argtypes = [P, P]
    if hasattr(L, "kad_snapshot_paths"):  # (absent from libraries of older revisions: A/B runs)
        L.kad_snapshot_paths.argtypes = [P, P]
    if hasattr(L, "kad_route_eval"):  # (absent from libraries of older revisions: A/B runs)
        L.kad_route_eval.argtypes = [P, ctypes.c_int32, ctypes.c_int32, P]
        L.kad_last_route.argtypes = [P, P]
        L.kad_route_variant_name.argtypes = [ctypes.c_int32]
        L.kad_route_variant_name.restype = ctypes.c_char_p
    L.kad_result_diff.argtypes = [P, P, P]
    L.kad_schedule_batch.argtypes = [P, P, P, SZ, P]
    L.kad_select_rows.argtypes = [P, I, P, P, P, U32, P, P, P]
    L.kad_plan_rows.argtypes = [P, I, P, P, P, P, P, P, P, P, P, P, P, P]
    L.kad_debug_scores.argtypes = [P, P, P, P]
    if hasattr(L, "kad_explain"):  # (absent from libraries of older revisions: A/B runs)
        L.kad_explain.argtypes = [P, P, P, I, P, I, P]
        L.kad_explain_timing.argtypes = [P, P]
    if hasattr(L, "kad_override_match"):  # (absent from libraries of older revisions: A/B runs)
        L.kad_override_policies_upload.argtypes = [P, P, SZ]
        L.kad_override_policies_check.argtypes = [P, SZ, P, SZ]
        L.kad_override_match.argtypes = [P, P, P]
        L.kad_override_timing.argtypes = [P, P]
    for name, (main, check, route_in, force) in _CONSUMER_ABI.items():
        if not hasattr(L, main):  # (absent from libraries of older revisions: A/B runs)
            continue
        getattr(L, main).argtypes = [P, P, P]
        getattr(L, f"kad_{name}_check").argtypes = [P, P, *check]
        getattr(L, f"kad_{name}_timing").argtypes = [P, P]
        getattr(L, f"kad_{name}_route_eval").argtypes = [*route_in, P]
        getattr(L, f"kad_{name}_last_route").argtypes = [P, P]
        if force is not None:
            getattr(L, f"kad_{name}_debug_route").argtypes = [P, *force]
    if hasattr(L, "kad_monitor_reserve"):  # (absent from libraries of older revisions: A/B runs)
        L.kad_monitor_reserve.argtypes = [P, _I64]
        L.kad_monitor_load.argtypes = [P, _I32] + [P] * 8
        L.kad_monitor_read.argtypes = [P, _I32] + [P] * 8
        L.kad_monitor_clear.argtypes = [P]
        L.kad_monitor_info.argtypes = [P, P]
    if hasattr(L, "kad_dispatch_decide"):
        L.kad_dispatch_decide.argtypes = [ctypes.c_uint32, ctypes.c_int32, ctypes.c_uint32, ctypes.c_uint32, P]
    if hasattr(L, "kad_deletion_finish"):  # (absent from libraries of older revisions: A/B runs)
        L.kad_deletion_finish.argtypes = [P, P, P, P]
        L.kad_deletion_decide.argtypes = [ctypes.c_uint32, ctypes.c_int32, ctypes.c_uint32, P]
    L.kad_debug_inject_fault.argtypes = [P, I]
    L.kad_debug_plan_force_workspace.argtypes = [P, I]
    L.kad_trigger_suffix_upload.argtypes = [P, P, SZ]
    L.kad_trigger_prefixes_upload.argtypes = [P, I, P, P]
    L.kad_trigger_run.argtypes = [P]
    L.kad_trigger_timing.argtypes = [P, P]
    L.kad_trigger_download.argtypes = [P, P]
    L.kad_trigger_hashes.argtypes = [P, I, P, P, P, SZ, P]
    L.kad_host_alloc.argtypes = [SZ, ctypes.POINTER(P)]
    L.kad_host_free.argtypes = [P]
    _bind_group(L, P, I, SZ)
    _lib = L
    return L


def _bind_group(L, P, I, SZ):
    """The kad_group_* entry points (ABI 3). A library built from an older revision for a same-box A/B run
    (scripts/build_old.sh) may lack them: its Context still works, GroupContext raises on first use.
    tests/test_abi.py checks that the product library exports every declared symbol."""
    if not hasattr(L, "kad_group_create"):
        return
    L.kad_group_create.argtypes = [P, I, ctypes.POINTER(P)]
    L.kad_group_destroy.argtypes = [P]
    L.kad_group_last_error.argtypes = [P]
    L.kad_group_last_error.restype = ctypes.c_char_p
    L.kad_group_size.argtypes = [P]
    L.kad_group_snapshot_upload.argtypes = [P, P, SZ]
    L.kad_group_snapshot_update.argtypes = [P, P, SZ]
    L.kad_group_batch_upload.argtypes = [P, P, SZ]
    L.kad_group_schedule.argtypes = [P, P]
    L.kad_group_sync.argtypes = [P]
    L.kad_group_results_download.argtypes = [P, P]
    L.kad_group_schedule_batch.argtypes = [P, P, P, SZ, P]
    L.kad_group_ranges.argtypes = [P, P, P]
    L.kad_group_path_counts.argtypes = [P, P]
    L.kad_group_set_timing.argtypes = [P, I]
    L.kad_group_member.argtypes = [P, I, ctypes.POINTER(P)]
    L.kad_batch_split.argtypes = [P, SZ, I, P, P]


class _HostBlock:
    """One kad_host_alloc block; freed when the last array viewing it goes away."""

    def __init__(self, nbytes: int):
        self.L = load_library()
        p = ctypes.c_void_p()
        rc = self.L.kad_host_alloc(nbytes, ctypes.byref(p))
        if rc != 0 or not p.value:
            raise KadError(rc, f"kad_host_alloc({nbytes}) failed")
        self.p = p.value

    def __del__(self):
        if getattr(self, "p", None):
            self.L.kad_host_free(self.p)
            self.p = None


def host_array(n: int, dtype) -> np.ndarray:
    """A page-locked numpy array of n elements (kad_host_alloc): D2H / H2D copies DMA straight into it."""
    dt = np.dtype(dtype)
    nbytes = max(1, n) * dt.itemsize
    blk = _HostBlock(nbytes)
    buf = (ctypes.c_uint8 * nbytes).from_address(blk.p)
    buf._owner = blk  # the array's base chain keeps the block alive
    return np.frombuffer(buf, dtype=dt, count=max(1, n))


def _p(a: Optional[np.ndarray]):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


# ---- the consumer calls' table-driven halves: every *_route_eval, *_args and *_check below is one line over these
def _route_eval(name: str, fields, *args, error=None) -> dict:
    """kad_<name>_route_eval on ``args``: the record as a dict of ``fields``."""
    fn = f"kad_{name}_route_eval"
    out = (ctypes.c_int32 * len(fields))()
    rc = getattr(load_library(), fn)(*args, out)
    if rc != 0:
        raise ValueError(f"{fn}: {rc}") if error is None else error(rc, fn)
    return dict(zip(fields, out))


def _flat(table, arrays, required=False) -> dict:
    """The arrays of ``table``'s rows (name, dtype, ...) as contiguous 1-d arrays of their dtype."""
    return {k: np.ascontiguousarray(arrays[k], dt).reshape(-1) for k, dt, *_ in table if required or k in arrays}


def _call_args(batch_cls, view_cls, counts, ins, outs, a: dict, n: dict):
    """(batch, view, the input arrays, the output arrays by name) of one consumer call. ``counts`` lead the batch,
    then one pointer per row of ``ins`` (null for an array that ``a`` lacks or that is empty). An output of ``outs``
    has n[its name] elements, else n[its third column], and is allocated with one at least; one with neither is
    left null."""
    size = {k: n.get(k, n.get(dim)) for k, _, dim in outs}
    out = {k: np.zeros(max(1, size[k]), dt) for k, dt, _ in outs if size[k] is not None}
    b = batch_cls(*counts, *(a[k].ctypes.data if k in a and len(a[k]) else None for k, *_ in ins))
    v = view_cls(*(out[k].ctypes.data if k in out else None for k, _, _ in outs))
    return b, v, a, {k: o[:size[k]] for k, o in out.items()}


def _check(name: str, args, *extra) -> int:
    """kad_<name>_check on the (batch, view, ...) of an *_args function."""
    b, v = args[:2]
    return getattr(load_library(), f"kad_{name}_check")(ctypes.byref(b), ctypes.byref(v), *extra)


FOLLOWER_ROUTE = ("path", "words", "threads", "grid", "lds", "stride")  # kad_follower_route_eval's record


def _follower_route_dict(d: dict) -> dict:
    d["path"] = ("WAVE", "BLOCK")[d["path"]]
    return d


def follower_route_eval(n_ids: int, n_followers: int, n_cu: int = 256) -> dict:
    """kad_follower_route_eval: the launch decision of a follower_union (needs no GPU)."""
    return _follower_route_dict(_route_eval("follower", FOLLOWER_ROUTE, n_ids, n_followers, n_cu))


def follower_args(n_ids: int, followers, leaders=None, keep=None, sched=None, n_leaders=None,
                  emit_all: bool = False, capacity: int = 0):
    """The kad_follower_batch / kad_follower_view of one call, with the arrays that back them.

    ``followers``: (fol_off[F + 1], fol_leader[], cur_off[F + 1], cur_cluster[], cur_has[F]); ``leaders``:
    (lead_off[n_leaders + 1], lead_cluster[]) or None for resident mode (leader i = unit i of the last
    schedule()); ``keep`` / ``sched``: (off, ids) CSRs or None; ``n_leaders`` defaults to the rows of
    ``leaders``, else of ``keep`` (resident mode without keep: pass it). Returns (batch, view, the int32 /
    uint8 arrays the batch points to, the output arrays by name)."""
    i32 = lambda a: np.ascontiguousarray(a, np.int32).reshape(-1)  # noqa: E731
    fo, fl, co, cc = (i32(a) for a in followers[:4])
    ch = np.ascontiguousarray(followers[4], np.uint8).reshape(-1)
    F = len(ch)
    pairs = [None if p is None else (i32(p[0]), i32(p[1])) for p in (leaders, sched, keep)]
    if n_leaders is None:
        src = pairs[0] or pairs[2]
        if src is None:
            raise ValueError("resident mode without keep: n_leaders is required")
        n_leaders = len(src[0]) - 1
    out = {"changed": np.zeros(max(1, F), np.uint8), "count": np.zeros(max(1, F), np.int32),
           "out_off": np.zeros(F + 1, np.int64), "out_cluster": np.zeros(max(1, int(capacity)), np.int32)}
    ptr = lambda a: a.ctypes.data if len(a) else None  # noqa: E731
    flat = []
    for p in pairs:
        flat += [None, None] if p is None else [p[0].ctypes.data, ptr(p[1])]
    b = FollowerBatch(int(n_ids), int(n_leaders), F, 1 if emit_all else 0, *flat, fo.ctypes.data, ptr(fl),
                      co.ctypes.data, ptr(cc), ch.ctypes.data if F else None, int(capacity))
    v = FollowerView(*(out[k].ctypes.data for k in ("changed", "count", "out_off", "out_cluster")))
    return b, v, (fo, fl, co, cc, ch, pairs), out


def follower_check(n_clusters: int, n_units: int, n_ids: int, followers, **kw) -> int:
    """kad_follower_check: kad_follower_union's validation of :func:`follower_args` arguments against a snapshot
    of ``n_clusters`` clusters and a scheduled batch of ``n_units`` units (-1: none); no GPU. Returns the code."""
    return _check("follower", follower_args(n_ids, followers, **kw), n_clusters, n_units)


MIGRATE_ROUTE = ("width", "long_min", "threads", "grid", "long_grid", "stride", "obj_width", "obj_grid")


def migrate_route_eval(n_segments: int, n_pods: int, n_long: int, n_objects: int, n_cu: int = 256) -> dict:
    """kad_migrate_route_eval: the launch decision of a migrate_estimate (needs no GPU)."""
    return _route_eval("migrate", MIGRATE_ROUTE, n_segments, n_pods, n_long, n_objects, n_cu)


_MIGRATE_IN = (("obj_seg_off", np.int32), ("obj_threshold_ns", np.int64), ("seg_cluster", np.int32),
               ("seg_desired", np.int64), ("seg_flags", np.uint8), ("seg_pod_off", np.int64), ("pod_t_ns", np.int64),
               ("pod_flags", np.uint8), ("old_off", np.int32), ("old_cluster", np.int32), ("old_cap", np.int64))
_MIGRATE_OUT = (("uns", np.int32, "S"), ("next_cross", np.int64, "S"), ("cap", np.int64, "S"), ("changed", np.uint8, "O"),
                ("n_written", np.int32, "O"), ("retry_after", np.int64, "O"), ("backoff", np.uint8, "O"))


def migrate_args(n_ids: int, now_ns: int, **arrays):
    """The kad_migrate_batch / kad_migrate_view of one call with the arrays that back them (the batch's
    fields by name; the counts are taken from the arrays as they are, so that a malformed batch reaches the
    library's validation). Returns (batch, view, the input arrays, the output arrays by name)."""
    a = _flat(_MIGRATE_IN, arrays, required=True)
    O_, S_ = len(a["obj_threshold_ns"]), len(a["seg_cluster"])
    counts = (int(n_ids), O_, S_, len(a["old_cluster"]), len(a["pod_t_ns"]), int(now_ns))
    return _call_args(MigrateBatch, MigrateView, counts, _MIGRATE_IN, _MIGRATE_OUT, a, {"O": O_, "S": S_})


def migrate_check(n_clusters: int, n_ids: int, now_ns: int, **arrays) -> int:
    """kad_migrate_check: kad_migrate_estimate's validation of :func:`migrate_args` arguments against a
    snapshot of ``n_clusters`` clusters; no GPU. Returns the code."""
    return _check("migrate", migrate_args(n_ids, now_ns, **arrays), n_clusters)


CSTAT_ROUTE = ("node_width", "pod_width", "long_min", "threads", "node_grid", "pod_grid", "long_grid", "chunk_grid")


def cstat_route_eval(n_clusters: int, n_long: int, short_nodes: int, short_pods: int, n_chunks: int,
                     n_cu: int = 256) -> dict:
    """kad_cstat_route_eval: the launch decision of a cluster_resources (needs no GPU)."""
    return _route_eval("cstat", CSTAT_ROUTE, n_clusters, n_long, short_nodes, short_pods, n_chunks, n_cu)


_CSTAT_IN = (("cl_node_off", np.int64), ("node_flags", np.uint8), ("node_ent_off", np.int64), ("nent_res", np.uint8),
             ("nent_val", np.int64), ("cl_pod_off", np.int64), ("pod_flags", np.uint8), ("pod_ent_off", np.int64),
             ("pent_res", np.uint8), ("pent_kind", np.uint8), ("pent_val", np.int64))
_CSTAT_OUT = (("alloc", np.int64, "KR"), ("avail", np.int64, "KR"), ("has", np.uint64, "K"), ("sched_nodes", np.int64, "K"))


def cstat_args(n_res: int, **arrays):
    """The kad_cstat_batch / kad_cstat_view of one call with the arrays that back them (the batch's fields by
    name; the counts are taken from the arrays as they are, so that a malformed batch reaches the library's
    validation). Returns (batch, view, the input arrays, the output arrays by name)."""
    a = _flat(_CSTAT_IN, arrays, required=True)
    K = max(0, len(a["cl_node_off"]) - 1)
    counts = (K, int(n_res), len(a["node_flags"]), len(a["pod_flags"]), len(a["nent_val"]), len(a["pent_val"]))
    return _call_args(CstatBatch, CstatView, counts, _CSTAT_IN, _CSTAT_OUT, a, {"K": K, "KR": K * max(0, int(n_res))})


def cstat_check(n_res: int, **arrays) -> int:
    """kad_cstat_check: kad_cluster_resources' validation of :func:`cstat_args` arguments; no GPU. Returns the
    code."""
    return _check("cstat", cstat_args(n_res, **arrays))


SAGG_ROUTE = ("width", "long_min", "threads", "grid", "long_grid", "stride")
SAGG_DEPLOYMENT, SAGG_JOB = 0, 1
SAGG_NV = {SAGG_DEPLOYMENT: 5, SAGG_JOB: 3}    # int32 rows of seg_vals / sums
SAGG_NOLD = {SAGG_DEPLOYMENT: 6, SAGG_JOB: 5}  # int64 rows of old_vals


def sagg_route_eval(n_objects: int, n_long: int, short_segments: int, n_cu: int = 256) -> dict:
    """kad_sagg_route_eval: the launch decision of a status_aggregate (needs no GPU)."""
    return _route_eval("sagg", SAGG_ROUTE, n_objects, n_long, short_segments, n_cu)


# (name, dtype, the kind it belongs to: 0 Deployment, 1 Job, 2 both)
_SAGG_IN = (("obj_seg_off", np.int32, 2), ("obj_flags", np.uint8, 2), ("obj_generation", np.int64, 0),
            ("obj_observed", np.int64, 0), ("old_vals", np.int64, 2), ("seg_vals", np.int32, 2), ("seg_flags", np.uint8, 2),
            ("seg_observed", np.int64, 0), ("seg_synced", np.int64, 0), ("seg_start", np.int64, 1), ("seg_done", np.int64, 1))
_SAGG_OUT = (("sums", np.int32, 2), ("changed", np.uint8, 2), ("observed", np.int64, 0), ("start_min", np.int64, 1),
             ("done_max", np.int64, 1), ("n_done", np.int32, 1), ("n_failed", np.int32, 1), ("finished", np.uint8, 1))


def sagg_args(kind: int, **arrays):
    """The kad_sagg_batch / kad_sagg_view of one call with the arrays that back them (the batch's fields by name;
    the counts are taken from the arrays as they are, so that a malformed batch reaches the library's
    validation; the other kind's arrays are left null). Returns (batch, view, the input arrays, the output
    arrays by name: ``sums`` as [NV, O])."""
    mine = (2, 1 if kind == SAGG_JOB else 0)
    a = _flat([row for row in _SAGG_IN if row[2] in mine], arrays)
    O_, S_ = len(a["obj_flags"]), len(a["seg_flags"])
    nv = SAGG_NV.get(kind, 5)
    n = {"sums": nv * O_, **{which: O_ for which in mine}}
    b, v, a, res = _call_args(SaggBatch, SaggView, (int(kind), O_, S_, 0), _SAGG_IN, _SAGG_OUT, a, n)
    res["sums"] = res["sums"].reshape(nv, O_)
    return b, v, a, res


def sagg_check(kind: int, **arrays) -> int:
    """kad_sagg_check: kad_status_aggregate's validation of :func:`sagg_args` arguments; no GPU. Returns the
    code."""
    return _check("sagg", sagg_args(kind, **arrays))


ROLLOUT_ROUTE = ("width", "long_min", "threads", "grid", "long_grid", "stride", "serial")
ROLLOUT_NV = 10  # int32 rows of tgt_vals


def rollout_route_eval(n_objects: int, n_long: int, short_targets: int, n_serial: int = 0, n_cu: int = 256) -> dict:
    """kad_rollout_route_eval: the launch decision of a rollout_plan (needs no GPU)."""
    return _route_eval("rollout", ROLLOUT_ROUTE, n_objects, n_long, short_targets, n_serial, n_cu)


_ROLLOUT_IN = (("obj_tgt_off", np.int32), ("obj_max_surge", np.int32), ("obj_max_unavailable", np.int32),
               ("obj_replicas", np.int32), ("obj_flags", np.uint8), ("tgt_vals", np.int32), ("tgt_flags", np.uint8))
_ROLLOUT_OUT = (("replicas", np.int32, 1), ("max_surge", np.int32, 1), ("max_unavailable", np.int32, 1),
                ("plan_flags", np.uint8, 1), ("action", np.uint8, 1), ("status", np.uint8, 0))


def rollout_args(**arrays):
    """The kad_rollout_batch / kad_rollout_view of one call with the arrays that back them (the batch's fields by
    name; the counts are taken from obj_flags and tgt_flags as they are, so that a malformed batch reaches the
    library's validation). Returns (batch, view, the input arrays, the output arrays by name)."""
    a = _flat(_ROLLOUT_IN, arrays)
    n = (len(a["obj_flags"]), len(a["tgt_flags"]))
    return _call_args(RolloutBatch, RolloutView, n, _ROLLOUT_IN, _ROLLOUT_OUT, a, dict(enumerate(n)))


def rollout_check(**arrays):
    """kad_rollout_check: kad_rollout_plan's validation of :func:`rollout_args` arguments; no GPU. Returns (the code,
    nowrap[O]: the objects the device plans with prefix sums)."""
    args = rollout_args(**arrays)
    O_ = args[0].n_objects
    nowrap = np.zeros(max(1, O_), np.uint8)
    return _check("rollout", args, nowrap.ctypes.data), nowrap[:max(0, O_)]


DISPATCH_ROUTE = ("words", "threads", "grid", "lds", "stride")
DISPATCH_MAX_CLUSTERS = 16384


def dispatch_route_eval(n_clusters: int, n_objects: int, n_cu: int = 256) -> dict:
    """kad_dispatch_route_eval: the launch decision of a dispatch_plan (needs no GPU)."""
    return _route_eval("dispatch", DISPATCH_ROUTE, n_clusters, n_objects, n_cu, error=KadError)


def dispatch_decide(cluster_flags: int, selected: bool, ob_flags: int = 0, obj_flags: int = 0):
    """kad_dispatch_decide: (op, status, recheck) of one (object, cluster) pair as the kernel decides it (no GPU)."""
    out = (ctypes.c_uint8 * 3)()
    rc = load_library().kad_dispatch_decide(cluster_flags, 1 if selected else 0, ob_flags, obj_flags, out)
    if rc != 0:
        raise KadError(rc, "kad_dispatch_decide")
    return int(out[0]), int(out[1]), bool(out[2])


_DISPATCH_IN = (("cluster_flags", np.uint8), ("obj_flags", np.uint8), ("obj_ns", np.int32), ("obj_pl_off", np.int32),
                ("pl_cluster", np.int32), ("ns_pl_off", np.int32), ("ns_cluster", np.int32), ("obj_ob_off", np.int32),
                ("ob_cluster", np.int32), ("ob_flags", np.uint8), ("out_off", np.int64))
_DISPATCH_OUT = (("out_cluster", np.int32, 1), ("out_op", np.uint8, 1), ("out_status", np.uint8, 1),
                 ("count", np.int32, 0), ("n_ops", np.int32, 0), ("n_selected", np.int32, 0), ("obj_result", np.uint8, 0))


def dispatch_args(fill: int = 0, **arrays):
    """The kad_dispatch_batch / kad_dispatch_view of one call with the arrays that back them (the batch's fields by
    name; the counts are taken from cluster_flags, obj_flags and ns_pl_off as they are, so that a malformed batch
    reaches the library's validation; ``n_clusters`` overrides the first). Every byte of the three entry arrays
    starts as ``fill``. Returns (batch, view, the input arrays, the output arrays by name)."""
    a = _flat(_DISPATCH_IN, arrays)
    C = int(arrays.get("n_clusters", len(a["cluster_flags"])))
    O, N = len(a["obj_flags"]), max(0, len(a["ns_pl_off"]) - 1)
    oo = a["out_off"]
    cap = int(oo[-1]) if len(oo) == O + 1 and len(oo) and 0 <= int(oo[-1]) < 2 ** 40 else 0
    b, v, a, out = _call_args(DispatchBatch, DispatchView, (C, O, N), _DISPATCH_IN, _DISPATCH_OUT, a, {0: O, 1: cap})
    if fill:
        for k, _, dim in _DISPATCH_OUT:
            if dim:
                out[k].view(np.uint8)[:] = fill
    return b, v, a, out


def dispatch_check(**arrays) -> int:
    """kad_dispatch_check: kad_dispatch_plan's validation of :func:`dispatch_args` arguments; no GPU."""
    return _check("dispatch", dispatch_args(**arrays))


DELETION_ROUTE = ("width", "long_min", "threads", "grid", "long_grid", "stride", "lds")  # both calls' record


def deletion_route_eval(n_clusters: int, n_objects: int, n_long: int, short_items: int, n_cu: int = 256) -> dict:
    """kad_deletion_route_eval: the launch decision of a deletion_plan (needs no GPU)."""
    return _route_eval("deletion", DELETION_ROUTE, n_clusters, n_objects, n_long, short_items, n_cu, error=KadError)


def deletion_finish_route_eval(n_clusters: int, n_objects: int, n_long: int, short_items: int, n_cu: int = 256) -> dict:
    """kad_deletion_finish_route_eval: the launch decision of a deletion_finish (needs no GPU)."""
    return _route_eval("deletion_finish", DELETION_ROUTE, n_clusters, n_objects, n_long, short_items, n_cu, error=KadError)


def deletion_decide(obj_flags: int, cluster_ready: bool, ob_flags: int = 0):
    """kad_deletion_decide: (op, remaining, retrieval_failed) of one (object, observed cluster) pair as both kernels
    decide it (no GPU)."""
    out = (ctypes.c_uint8 * 3)()
    rc = load_library().kad_deletion_decide(obj_flags, 1 if cluster_ready else 0, ob_flags, out)
    if rc != 0:
        raise KadError(rc, "kad_deletion_decide")
    return int(out[0]), bool(out[1]), bool(out[2])


_DELETION_IN = (("cluster_flags", np.uint8), ("obj_flags", np.uint8), ("obj_ob_off", np.int32), ("ob_cluster", np.int32),
                ("ob_flags", np.uint8))
_DELETION_OUT = (("out_op", np.uint8, 1), ("n_ops", np.int32, 0), ("n_remaining", np.int32, 0),
                 ("n_retrieval_failed", np.int32, 0), ("obj_pre", np.uint8, 0), ("obj_first", np.uint8, 0))
_DELETION_RES = (("op_ok", np.uint8), ("obj_wait", np.uint8), ("chk_off", np.int32), ("chk_cluster", np.int32),
                 ("chk_flags", np.uint8), ("chk_cluster_flags", np.uint8))
_DELETION_FIN_OUT = (("obj_status", np.uint8, 0), ("obj_reason", np.uint8, 0), ("obj_then", np.uint8, 0),
                     ("n_failed_ops", np.int32, 0), ("n_failed_checks", np.int32, 0))


def _deletion_counts(a: dict, arrays: dict):
    C = int(arrays.get("n_clusters", len(a["cluster_flags"]) if "cluster_flags" in a else 0))
    O = len(a["obj_flags"]) if "obj_flags" in a else 0
    oo = a.get("obj_ob_off")
    B = int(oo[-1]) if oo is not None and len(oo) == O + 1 and 0 <= int(oo[-1]) < 2 ** 31 else 0
    return C, O, B


def _filled(out: dict, fill: int) -> dict:
    if fill:
        for o in out.values():
            o.view(np.uint8)[:] = fill
    return out


def deletion_args(fill: int = 0, pad: int = 0, **arrays):
    """The kad_deletion_batch / kad_deletion_view of one call with the arrays that back them (the batch's fields by
    name; the counts are taken from cluster_flags and obj_flags as they are, so that a malformed batch reaches the
    library's validation; ``n_clusters`` overrides the first). Every output has ``pad`` more elements than the call
    writes and every byte of it starts as ``fill``. Returns (batch, view, the input arrays, the output arrays by
    name)."""
    a = _flat(_DELETION_IN, arrays)
    C, O, B = _deletion_counts(a, arrays)
    b, v, a, out = _call_args(DeletionBatch, DeletionView, (C, O), _DELETION_IN, _DELETION_OUT, a, {0: O + pad, 1: B + pad})
    return b, v, a, _filled(out, fill)


def deletion_finish_args(fill: int = 0, pad: int = 0, **arrays):
    """The kad_deletion_batch / kad_deletion_finish_view / kad_deletion_results of one kad_deletion_finish, as
    :func:`deletion_args` builds the plan's. Returns (batch, view, the arrays kept alive, the output arrays by name,
    results)."""
    a = _flat(_DELETION_IN, arrays)
    r = _flat(_DELETION_RES, arrays)
    C, O, B = _deletion_counts(a, arrays)
    # the library gets pointers only: an array it reads by the batch's counts must have that many elements (an empty
    # one is passed as missing and rejected by the validation)
    for k, n in (("chk_cluster_flags", len(a["cluster_flags"]) if "cluster_flags" in a else 0), ("op_ok", B), ("obj_wait", O)):
        if k in r and len(r[k]) not in (0, n):
            raise ValueError(f"{k} has {len(r[k])} elements, the batch's counts say {n}")
    b, v, a, out = _call_args(DeletionBatch, DeletionFinishView, (C, O), _DELETION_IN, _DELETION_FIN_OUT, a, {0: O + pad})
    res = DeletionResults(*(r[k].ctypes.data if k in r and len(r[k]) else None for k, _ in _DELETION_RES))
    return b, v, (a, r), _filled(out, fill), res


def deletion_check(**arrays) -> int:
    """kad_deletion_check: kad_deletion_plan's validation of :func:`deletion_args` arguments; no GPU."""
    return _check("deletion", deletion_args(**arrays))


def deletion_finish_check(**arrays) -> int:
    """kad_deletion_finish_check: kad_deletion_finish's validation of :func:`deletion_finish_args` arguments; no GPU."""
    args = deletion_finish_args(**arrays)
    return _check("deletion_finish", args, ctypes.byref(args[4]))


POLICYRC_ROUTE = ("path", "bins", "threads", "grid", "vec", "apply_grid")
POLICYRC_PATHS = ("LDS", "GLOBAL")  # the record's path; policyrc_debug_route forces 1 + its index
PRC_POL_EXISTS, PRC_POL_ENQUEUED = 1, 2
PRC_FLAGGED, PRC_UPDATE, PRC_NEGATIVE = 1, 2, 4


def policyrc_route_eval(n_policies: int, n_ids: int, n_cu: int = 256) -> dict:
    """kad_policyrc_route_eval: the launch decision of a policyrc_count over n_ids = n_dec + n_inc ids (needs no
    GPU)."""
    return _route_eval("policyrc", POLICYRC_ROUTE, n_policies, n_ids, n_cu, error=KadError)


_POLICYRC_IN = (("dec_ids", np.int32), ("inc_ids", np.int32), ("count", np.int64), ("stored_typed", np.int64),
                ("stored_rest", np.int64), ("stored_total", np.int64), ("pol_flags", np.uint8))
_POLICYRC_OUT = (("new_count", np.int64, 0), ("new_total", np.int64, 0), ("state", np.uint8, 0), ("n_negative", np.int32, 1))


def policyrc_args(**arrays):
    """The kad_policyrc_batch / kad_policyrc_view of one call with the arrays that back them (the batch's fields by
    name; the counts are taken from pol_flags, dec_ids and inc_ids as they are, so that a malformed batch reaches
    the library's validation; ``n_policies``, ``n_dec``, ``n_inc`` and ``reserved`` override them). Returns (batch,
    view, the input arrays, the output arrays by name)."""
    a = _flat(_POLICYRC_IN, arrays)
    counts = tuple(int(arrays.get(k, len(a[src]) if src in a else 0))
                   for k, src in (("n_policies", "pol_flags"), ("n_dec", "dec_ids"), ("n_inc", "inc_ids")))
    P = max(0, counts[0], len(a["pol_flags"]) if "pol_flags" in a else 0)
    return _call_args(PolicyrcBatch, PolicyrcView, counts + (int(arrays.get("reserved", 0)),), _POLICYRC_IN,
                      _POLICYRC_OUT, a, {0: P, 1: 1})


def policyrc_check(**arrays) -> int:
    """kad_policyrc_check: kad_policyrc_count's validation of :func:`policyrc_args` arguments; no GPU."""
    return _check("policyrc", policyrc_args(**arrays))


SYNC_NU_ROUTE = ("threads", "grid", "stride")
SYNC_FIN_ROUTE = ("width", "long_min", "threads", "grid", "long_grid", "stride")


def sync_needs_update_route_eval(n_rows: int, n_cu: int = 256) -> dict:
    """kad_sync_needs_update_route_eval: the launch decision of a sync_needs_update (needs no GPU)."""
    return _route_eval("sync_needs_update", SYNC_NU_ROUTE, n_rows, n_cu, error=KadError)


def sync_finish_route_eval(n_objects: int, n_long: int, short_items: int, n_cu: int = 256) -> dict:
    """kad_sync_finish_route_eval: the launch decision of a sync_finish (needs no GPU)."""
    return _route_eval("sync_finish", SYNC_FIN_ROUTE, n_objects, n_long, short_items, n_cu, error=KadError)


_SYNC_NU_IN = (("row_obj", np.int32), ("row_cluster", np.int32), ("row_target", np.int32), ("row_flags", np.uint8),
               ("obj_flags", np.uint8), ("rec_off", np.int32), ("rec_cluster", np.int32), ("rec_version", np.int32),
               ("ver_flags", np.uint8))
_SYNC_NU_OUT = (("needs_update", np.uint8, 0), ("recorded", np.int32, 0))
_SYNC_FIN_IN = (("obj_flags", np.uint16), ("reason_in", np.int32), ("cond_reason", np.int32), ("sel_off", np.int32),
                ("sel_cluster", np.int32), ("ent_off", np.int32), ("ent_cluster", np.int32), ("ent_status", np.uint8),
                ("ent_version", np.int32), ("oldv_off", np.int32), ("oldv_cluster", np.int32), ("oldv_version", np.int32),
                ("olds_off", np.int32), ("olds_cluster", np.int32), ("olds_status", np.uint8), ("olds_gen", np.int64),
                ("ver_gen", np.int64), ("ver_flags", np.uint8), ("ver_off", np.int64), ("st_off", np.int64))
_SYNC_FIN_OUT = (("out_ver_cluster", np.int32, 1), ("out_ver_id", np.int32, 1), ("ver_count", np.int32, 0),
                 ("ver_write", np.uint8, 0), ("out_st_cluster", np.int32, 2), ("out_st_status", np.uint8, 2),
                 ("out_st_gen", np.int64, 2), ("st_count", np.int32, 0), ("obj_out", np.uint8, 0), ("reason_out", np.int32, 0))


def sync_needs_update_args(n_clusters: int, **arrays):
    """The kad_sync_nu_batch / kad_sync_nu_view of one call with the arrays that back them (the batch's fields by
    name; the other counts are taken from obj_flags, row_flags and ver_flags as they are, so that a malformed batch
    reaches the library's validation; ``n_versions`` overrides the last). Returns (batch, view, the input arrays, the
    output arrays by name)."""
    a = _flat(_SYNC_NU_IN, arrays)
    n = lambda k: len(a[k]) if k in a else 0  # noqa: E731
    counts = (int(n_clusters), n("obj_flags"), n("row_flags"), int(arrays.get("n_versions", n("ver_flags"))))
    return _call_args(SyncNuBatch, SyncNuView, counts, _SYNC_NU_IN, _SYNC_NU_OUT, a, {0: counts[2]})


def sync_needs_update_check(n_clusters: int, **arrays) -> int:
    """kad_sync_needs_update_check: the call's validation of :func:`sync_needs_update_args` arguments; no GPU."""
    return _check("sync_needs_update", sync_needs_update_args(n_clusters, **arrays))


def sync_finish_args(n_clusters: int, n_reasons: int, reason_check_clusters: int, reason_ns_not_federated: int, **arrays):
    """The kad_sync_fin_batch / kad_sync_fin_view of one call with the arrays that back them (the batch's fields by
    name; n_objects and n_versions are taken from obj_flags and ver_flags as they are, so that a malformed batch
    reaches the library's validation; ``n_versions`` overrides the second). Returns (batch, view, the input arrays,
    the output arrays by name)."""
    a = _flat(_SYNC_FIN_IN, arrays)
    n = lambda k: len(a[k]) if k in a else 0  # noqa: E731
    O = n("obj_flags")
    counts = (int(n_clusters), O, int(arrays.get("n_versions", n("ver_flags"))), int(n_reasons),
              int(reason_check_clusters), int(reason_ns_not_federated))

    def cap(k):
        off = a.get(k)
        return int(off[-1]) if off is not None and len(off) == O + 1 and 0 <= int(off[-1]) < 2 ** 31 else 0

    return _call_args(SyncFinBatch, SyncFinView, counts, _SYNC_FIN_IN, _SYNC_FIN_OUT, a,
                      {0: O, 1: cap("ver_off"), 2: cap("st_off")})


def sync_finish_check(n_clusters: int, n_reasons: int, reason_check_clusters: int, reason_ns_not_federated: int,
                      **arrays) -> int:
    """kad_sync_finish_check: kad_sync_finish's validation of :func:`sync_finish_args` arguments; no GPU."""
    return _check("sync_finish", sync_finish_args(n_clusters, n_reasons, reason_check_clusters,
                                                  reason_ns_not_federated, **arrays))


MONITOR_REC_ROUTE = ("width", "long_min", "threads", "grid", "long_grid", "stride")
MONITOR_REP_ROUTE = ("path", "bins", "threads", "grid", "vec", "wtiles")
MONITOR_PATHS = ("LDS", "GLOBAL")  # the record's path; monitor_report_debug_route forces 1 + its index
MONITOR_COLUMNS = ("creation", "last_update", "sync_success", "last_status_synced", "out_of_sync_ns")
MON_TIME_ZERO = -(1 << 62)


def monitor_reconcile_route_eval(n_objects: int, n_long: int, short_items: int, n_cu: int = 256) -> dict:
    """kad_monitor_reconcile_route_eval: the launch decision of a monitor_reconcile (needs no GPU)."""
    return _route_eval("monitor_reconcile", MONITOR_REC_ROUTE, n_objects, n_long, short_items, n_cu, error=KadError)


def monitor_report_route_eval(n_slots: int, n_types: int, n_cu: int = 256) -> dict:
    """kad_monitor_report_route_eval: the launch decision of a monitor_report (needs no GPU)."""
    return _route_eval("monitor_report", MONITOR_REP_ROUTE, n_slots, n_types, n_cu, error=KadError)


_MONITOR_IN = (("slot", np.int32), ("obj_flags", np.uint16), ("type_id", np.int32), ("creation_ns", np.int64),
               ("sync_success_ns", np.int64), ("fed_off", np.int32), ("fed_cluster", np.int32), ("fed_gen", np.int64),
               ("mem_off", np.int32), ("mem_cluster", np.int32), ("mem_gen", np.int64), ("last_off", np.int32),
               ("last_cluster", np.int32), ("last_gen", np.int64))
_MONITOR_OUT = (("result", np.uint8, 0), ("bits", np.uint8, 0), ("meter", np.int64, 1), ("would", np.int64, 2))
_MONITOR_REP_OUT = (("counters", np.int32, 0), ("type_sync", np.int32, 1), ("type_status", np.int32, 1),
                    ("sync_slot", np.int32, 2), ("sync_ms", np.int64, 2), ("status_slot", np.int32, 2),
                    ("status_ms", np.int64, 2), ("n_timers", np.int32, 3))


def monitor_reconcile_args(n_clusters: int, now_ns: int, **arrays):
    """The kad_monitor_batch / kad_monitor_view of one call with the arrays that back them (the batch's fields by
    name; n_objects is taken from obj_flags as it is, so that a malformed batch reaches the library's validation).
    Returns (batch, view, the input arrays, the output arrays by name)."""
    a = _flat(_MONITOR_IN, arrays)
    O = len(a["obj_flags"]) if "obj_flags" in a else 0
    return _call_args(MonitorBatch, MonitorView, (O, int(n_clusters), int(now_ns)), _MONITOR_IN, _MONITOR_OUT, a,
                      {0: O, 1: 5 * O, 2: 2 * O})


def monitor_reconcile_check(n_clusters: int, now_ns: int, **arrays) -> int:
    """kad_monitor_reconcile_check: the call's validation that needs no table; no GPU."""
    return _check("monitor_reconcile", monitor_reconcile_args(n_clusters, now_ns, **arrays))


def monitor_report_args(now_ns: int, n_types: int, timer_cap: int):
    """The kad_monitor_report_batch / kad_monitor_report_view of one call and its output arrays by name."""
    return _call_args(MonitorReportBatch, MonitorReportView, (int(now_ns), int(n_types), int(timer_cap)), (),
                      _MONITOR_REP_OUT, {}, {0: 14, 1: max(0, int(n_types)), 2: max(0, int(timer_cap)), 3: 2})


def monitor_report_check(now_ns: int, n_types: int, timer_cap: int) -> int:
    """kad_monitor_report_check: the call's validation that needs no table; no GPU."""
    return _check("monitor_report", monitor_report_args(now_ns, n_types, timer_cap))


REVISION_ROUTE = ("width", "long_min", "cmp_width", "hash_grid", "cmp_grid", "grid", "long_grid", "threads")


def revision_plan_route_eval(n_objects: int, n_hash: int, n_long: int, short_revs: int, n_pairs: int, pair_chunks: int,
                             n_cu: int = 256) -> dict:
    """kad_revision_plan_route_eval: the launch decision of a revision_plan (needs no GPU)."""
    return _route_eval("revision_plan", REVISION_ROUTE, n_objects, n_hash, n_long, short_revs, n_pairs, pair_chunks, n_cu,
                       error=KadError)


_REVISION_IN = (("limit", np.int64), ("collision", np.int32), ("obj_flags", np.uint8), ("patch_off", np.int64),
                ("patch_len", np.int32), ("blob", np.uint8), ("rev_off", np.int32), ("rev_data_off", np.int64),
                ("rev_data_len", np.int32), ("rev_revision", np.int64), ("rev_time", np.int64), ("rev_name_rank", np.int32),
                ("rev_flags", np.uint8), ("rev_hash", np.uint32), ("rev_lab_off", np.int32), ("rev_lab", np.int32),
                ("want_off", np.int32), ("want_lab", np.int32))
_REVISION_OUT = (("out_off", np.int64, 3), ("hash", np.uint32, 0), ("upd_hash", np.uint32, 0), ("upd_parsed", np.uint8, 0),
                 ("equal", np.uint8, 1), ("order", np.int32, 1), ("n_old", np.int32, 0), ("keep", np.int32, 0),
                 ("n_actions", np.int32, 0), ("last", np.int32, 0), ("rev_number", np.int64, 0), ("act_kind", np.uint8, 2),
                 ("act_rev", np.int32, 2))


def revision_plan_args(n_pairs: int, **arrays):
    """The kad_revision_batch / kad_revision_view of one call with the arrays that back them (the batch's fields by
    name; n_objects is taken from obj_flags and blob_len from blob as they are, so that a malformed batch reaches the
    library's validation; ``n_objects``, ``blob_len`` and ``action_capacity`` override them, the last defaulting to
    2 R + O). Returns (batch, view, the input arrays, the output arrays by name)."""
    a = _flat(_REVISION_IN, arrays)
    n = lambda k: len(a[k]) if k in a else 0  # noqa: E731
    O = int(arrays.get("n_objects", n("obj_flags")))
    R = n("rev_flags")
    cap = int(arrays.get("action_capacity", 2 * R + max(O, 0)))
    counts = (O, int(n_pairs), int(arrays.get("blob_len", n("blob"))), cap)
    return _call_args(RevisionBatch, RevisionView, counts, _REVISION_IN, _REVISION_OUT, a,
                      {0: max(O, 0), 1: R, 2: max(cap, 0), 3: max(O, 0) + 1})


def revision_plan_check(n_pairs: int, **arrays) -> int:
    """kad_revision_plan_check: kad_revision_plan's validation of :func:`revision_plan_args` arguments; no GPU."""
    return _check("revision_plan", revision_plan_args(n_pairs, **arrays))


class Context:
    """A kad_ctx: one HIP device, one stream, resident snapshot + batch."""

    def __init__(self, device: int = 0):
        self.device = device
        self.L = load_library()
        h = ctypes.c_void_p()
        rc = self.L.kad_ctx_create(device, ctypes.byref(h))
        if rc != 0:
            raise KadError(rc, f"kad_ctx_create(device={device}) failed (no GPU?)")
        self.h = h
        self.snap: Optional[Snapshot] = None
        self.batch: Optional[Batch] = None

    def close(self):
        if self.h:
            self.L.kad_ctx_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _chk(self, rc):
        if rc != 0:
            raise KadError(rc, self.L.kad_last_error(self.h).decode())

    # ---- the consumer calls' table-driven halves (the module's _CONSUMER_ABI names them)
    def _consume(self, fn: str, args) -> dict:
        """The consumer call ``fn`` on the (batch, view, inputs, outputs) of its *_args function → the outputs."""
        b, v, _keepalive, out = args
        self._chk(getattr(self.L, fn)(self.h, ctypes.byref(b), ctypes.byref(v)))
        return out

    def _timing(self, name: str, n: int):
        """kad_<name>_timing: its n device intervals in ms."""
        ms = (ctypes.c_float * n)()
        self._chk(getattr(self.L, f"kad_{name}_timing")(self.h, ms))
        return tuple(float(x) for x in ms)

    def _last_route(self, name: str, fields) -> dict:
        """kad_<name>_last_route: the record of kad_<name>_route_eval as a dict of ``fields``."""
        out = (ctypes.c_int32 * len(fields))()
        self._chk(getattr(self.L, f"kad_{name}_last_route")(self.h, out))
        return dict(zip(fields, out))

    def _debug_route(self, name: str, *force) -> None:
        self._chk(getattr(self.L, f"kad_{name}_debug_route")(self.h, *force))

    def upload_snapshot(self, snap: Snapshot):
        self._chk(self.L.kad_snapshot_upload(self.h, _p(snap.blob), snap.blob.nbytes))
        self.snap = snap

    def upload_snapshot_blob(self, blob: np.ndarray, snap: Optional[Snapshot] = None):
        """kad_snapshot_upload of a packed snapshot blob (e.g. received from the packing rank)."""
        blob = np.ascontiguousarray(blob, np.uint8)
        self._chk(self.L.kad_snapshot_upload(self.h, _p(blob), blob.nbytes))
        self.snap = snap

    def upload_snapshot_device(self, dev_ptr: int, nbytes: int, snap: Optional[Snapshot] = None):
        self._chk(self.L.kad_snapshot_upload_device(self.h, ctypes.c_void_p(dev_ptr), nbytes))
        self.snap = snap

    def inject_fault(self, where: int):
        """kad_debug_inject_fault (tests): 1 = the next snapshot upload / update fails in its derived-state
        rebuild."""
        self._chk(self.L.kad_debug_inject_fault(self.h, where))

    def plan_force_workspace(self, on):
        """kad_debug_plan_force_workspace (tests): plan_rows through the LDS-workspace planner (True / 1), the
        half-wave pair planner (2), or the default choice by row length (False / 0)."""
        self._chk(self.L.kad_debug_plan_force_workspace(self.h, int(on)))

    def update_snapshot(self, delta: SnapshotDelta):
        """kad_snapshot_update: patch the resident snapshot; the resident batch stays valid."""
        self._chk(self.L.kad_snapshot_update(self.h, _p(delta.blob), delta.blob.nbytes))

    def upload_batch(self, batch: Batch):
        chk = getattr(batch, "check_current", None)
        if chk is not None:
            chk()
        self._chk(self.L.kad_batch_upload(self.h, _p(batch.blob), batch.blob.nbytes))
        self.batch = batch

    def schedule(self, fwk: Framework):
        prof = fwk.to_c()
        self._chk(self.L.kad_schedule(self.h, ctypes.byref(prof)))

    def sync(self):
        self._chk(self.L.kad_sync(self.h))

    def set_timing(self, on: bool):
        """kad_set_timing: HIP event records around the stages of later schedule() calls."""
        self._chk(self.L.kad_set_timing(self.h, 1 if on else 0))

    def timing(self):
        ms = (ctypes.c_float * 3)()
        self._chk(self.L.kad_last_timing(self.h, ms))
        return float(ms[0]), float(ms[1]), float(ms[2])

    STAGES = ("req_mask", "prep", "main", "defer", "planner", "total", "rows")

    def stage_timing(self) -> dict:
        """kad_stage_timing: device ms per stage of the last timed schedule() (rows = schedule_row_kernel,
        defer = schedule_kernel over the defer list)."""
        ms = (ctypes.c_float * 7)()
        self._chk(self.L.kad_stage_timing(self.h, ms, 7))
        return {k: float(v) for k, v in zip(self.STAGES, ms)}

    DIFF_PLACEMENT, DIFF_OVERRIDES, DIFF_SKIP, DIFF_STICKY = 1, 2, 4, 8

    def result_diff(self, state: dict) -> np.ndarray:
        """kad_result_diff: per unit of the last schedule(), which parts of applySchedulingResult would change
        its object (KAD_DIFF_* flags). ``state``: objects.result_states(...) arrays."""
        W = len(state["place_has"])
        keep = {k: np.ascontiguousarray(v) for k, v in state.items() if isinstance(v, np.ndarray)}
        st = ResultState(W, *(_p(keep[k]) for k in ("place_off", "place_cluster", "place_has", "ovr_off", "ovr_cluster",
                                                    "ovr_value", "ovr_kind")))
        out = np.zeros(max(1, W), np.uint32)
        self._chk(self.L.kad_result_diff(self.h, ctypes.byref(st), _p(out)))
        return out[:W]

    def path_counts(self) -> dict:
        """kad_path_counts: units per kernel path of the last schedule()."""
        out = (ctypes.c_int32 * 4)()
        self._chk(self.L.kad_path_counts(self.h, out))
        return {"units": out[0], "full_kernel": out[1], "row_kernel": out[2], "planner_rows": out[3]}

    def snapshot_paths(self) -> dict:
        """kad_snapshot_paths: the resident snapshot's resource class and the kernel path it takes."""
        out = (ctypes.c_int32 * 5)()
        self._chk(self.L.kad_snapshot_paths(self.h, out))
        return {"resource_class": {2: "strict", 1: "relaxed", 0: "generic"}[out[0]], "exact_f64": bool(out[1]),
                "wide": bool(out[2]), "fold": bool(out[3]), "fitfold": bool(out[4])}

    def last_route(self) -> dict:
        """kad_last_route: what the last schedule() launched (route_eval's record, grids included)."""
        out = (ctypes.c_int32 * len(ROUTE_OUT))()
        self._chk(self.L.kad_last_route(self.h, out))
        return _route_dict(self.L, out)

    def copy_results_device(self, status_ptr: int, count_ptr: int, flags_ptr: int, cluster_ptr: int,
                            replicas_ptr: int):
        """kad_results_copy_device: results D2D into caller device buffers (e.g. torch tensors)."""
        v = ResultView(status_ptr, count_ptr, flags_ptr, cluster_ptr, replicas_ptr)
        self._chk(self.L.kad_results_copy_device(self.h, ctypes.byref(v)))

    def download(self, out: Optional[BatchResult] = None) -> BatchResult:
        """kad_results_download into fresh arrays, or into ``out`` (e.g. page-locked arrays reused across
        batches: BatchResult.pinned), which must be sized for the uploaded batch."""
        if out is None:
            res = BatchResult.empty(self.batch)
        else:  # views of the batch's sizes
            W, n = self.batch.W, max(1, self.batch.n_out_slots)
            arrs = ((out.status, W), (out.count, W), (out.flags, W), (out.cluster, n), (out.replicas, n))
            for (a, m), dt in zip(arrs, (np.int32, np.int32, np.uint32, np.int32, np.int64)):
                if a.dtype != dt:  # kad_results_download copies 4 or 8 bytes per element
                    raise ValueError(f"download buffer dtype {a.dtype}, kad_results_download writes {np.dtype(dt)}")
                if len(a) < m or not a.flags.c_contiguous:
                    raise ValueError("download buffers smaller than the uploaded batch")
            res = BatchResult(*(a[:m] for a, m in arrs), self.batch.out_off)
        v = ResultView(res.status.ctypes.data, res.count.ctypes.data, res.flags.ctypes.data, res.cluster.ctypes.data,
                       res.replicas.ctypes.data)
        self._chk(self.L.kad_results_download(self.h, ctypes.byref(v)))
        return res

    def schedule_batch(self, fwk: Framework, batch: Batch) -> BatchResult:
        """kad_schedule_batch: upload, schedule and download under one hold of the context lock."""
        chk = getattr(batch, "check_current", None)
        if chk is not None:
            chk()
        res = BatchResult.empty(batch)
        v = ResultView(res.status.ctypes.data, res.count.ctypes.data, res.flags.ctypes.data, res.cluster.ctypes.data,
                       res.replicas.ctypes.data)
        prof = fwk.to_c()
        self._chk(self.L.kad_schedule_batch(self.h, ctypes.byref(prof), _p(batch.blob), batch.blob.nbytes,
                                            ctypes.byref(v)))
        self.batch = batch
        return res

    def run(self, fwk: Framework, batch: Batch) -> BatchResult:
        self.upload_batch(batch)
        self.schedule(fwk)
        return self.download()

    def debug_scores(self, fwk: Framework):
        W, C = self.batch.W, self.snap.C
        feas = np.zeros(max(1, W * C), np.uint8)
        tot = np.zeros(max(1, W * C), np.int64)
        prof = fwk.to_c()
        self._chk(self.L.kad_debug_scores(self.h, ctypes.byref(prof), _p(feas), _p(tot)))
        return feas[:W * C].reshape(W, C), tot[:W * C].reshape(W, C)

    def explain(self, fwk: Framework, units=None, per_cluster: bool = False, fit_detail: bool = True
                ) -> FilterDiagnosis:
        """kad_explain: per listed unit of the uploaded batch (``units=None``: all of them), how many clusters
        each filter plugin of ``fwk`` rejected — each cluster counted for the first plugin that fails in the
        framework's order — and how many passed; ``per_cluster`` adds the rejecting plugin per cluster. Works
        before or after schedule() and changes nothing a later schedule() or download() sees."""
        W, C = self.batch.W, self.snap.C
        idx = np.arange(W, dtype=np.int32) if units is None else np.ascontiguousarray(units, np.int32).reshape(-1)
        n = len(idx)
        order = fwk.filter_order()
        ord_a = np.array(order or [0], np.int32)
        rej = np.zeros((max(1, n), 5), np.int32)
        feas = np.zeros(max(1, n), np.int32)
        fit = np.zeros((max(1, n), 3), np.int32) if fit_detail else None
        ff = np.zeros((max(1, n), max(1, C)), np.uint8) if per_cluster else None
        v = ExplainView(rej.ctypes.data, feas.ctypes.data, None if fit is None else fit.ctypes.data,
                        None if ff is None else ff.ctypes.data)
        prof = fwk.to_c()
        self._chk(self.L.kad_explain(self.h, ctypes.byref(prof), _p(ord_a), len(order), _p(idx) if n else None, n,
                                     ctypes.byref(v)))
        if ff is not None:  # the library wrote n rows of C bytes at the start of the buffer
            ff = ff.reshape(-1)[:n * C].reshape(n, C).copy()
        return FilterDiagnosis(idx, rej[:n], feas[:n], None if fit is None else fit[:n], ff, order, C)

    def explain_timing(self):
        """kad_explain_timing: device ms of the last explain() — (requirement rows, filter_explain_kernel)."""
        return self._timing("explain", 2)

    def upload_override_policies(self, policy_set):
        """kad_override_policies_upload: an overrides.PolicySet packed against the uploaded snapshot."""
        self._chk(self.L.kad_override_policies_upload(self.h, _p(policy_set.blob), policy_set.blob.nbytes))
        self.policy_set = policy_set

    def override_match(self, obj_policy, placed=None, rule_words: Optional[int] = None):
        """kad_override_match → (status[n], matched[n_slots][RW]). ``obj_policy``: [n][2] indices into the
        uploaded policy set (-1: none; column 0 the ClusterOverridePolicy). ``placed``: (place_off[n + 1],
        place_cluster[]) as snapshot cluster ids, or None for the placements of the last schedule(): the
        slots are then the batch's output slots followed by its CurrentClusters entries (sticky units)."""
        op = np.ascontiguousarray(obj_policy, np.int32).reshape(-1, 2)
        n = len(op)
        rw = rule_words if rule_words is not None else self.policy_set.rule_words(op)
        if placed is None:
            hdr = _pack.header_of(self.batch.blob, _pack.BatchHeader)
            cur_off = _pack.array_of(self.batch.blob, hdr, _pack.B_CUR_OFF, np.int32, hdr.n_units + 1)
            n_slots = int(hdr.n_out_slots) + int(cur_off[hdr.n_units])
            off = ids = None
        else:
            off = np.ascontiguousarray(placed[0], np.int32)
            ids = np.ascontiguousarray(placed[1], np.int32)
            n_slots = len(ids)
        status = np.zeros(max(1, n), np.int32)
        matched = np.zeros((max(1, n_slots), rw), np.uint32)
        b = OverrideBatch(n, rw, op.ctypes.data, None if off is None else off.ctypes.data,
                          None if ids is None or not len(ids) else ids.ctypes.data)
        v = OverrideView(status.ctypes.data, matched.ctypes.data)
        self._chk(self.L.kad_override_match(self.h, ctypes.byref(b), ctypes.byref(v)))
        return status[:n], matched[:n_slots]

    def override_timing(self):
        """kad_override_timing: device ms of the last override_match() — (the policy set's requirement rows,
        override_rule_rows_kernel, the status + match kernels)."""
        return self._timing("override", 3)

    def follower_union(self, n_ids: int, followers, leaders=None, keep=None, sched=None, n_leaders=None,
                       emit_all: bool = False, capacity: Optional[int] = None, retry: bool = True) -> dict:
        """kad_follower_union → {changed[F], count[F], out_off[F + 1], out_cluster[out_off[F]], calls}.
        Arguments as :func:`follower_args`. ``capacity``: elements of the first call's out_cluster (default: one
        per current-placement entry plus one per follower); when the library answers KAD_ENOSPC the call is
        repeated once with the out_off[F] slots it asked for (``retry=False``: the error is raised, with the
        valid changed / count / out_off of that call in ``KadError.partial``)."""
        F = len(followers[4])
        cap = int(capacity) if capacity is not None else len(followers[3]) + F
        for calls in (1, 2):
            b, v, keepalive, out = follower_args(n_ids, followers, leaders, keep, sched, n_leaders, emit_all, cap)
            rc = self.L.kad_follower_union(self.h, ctypes.byref(b), ctypes.byref(v))
            if rc == KAD_ENOSPC and retry and calls == 1:
                cap = int(out["out_off"][F])
                continue
            if rc != 0:
                e = KadError(rc, self.L.kad_last_error(self.h).decode())
                if rc == KAD_ENOSPC:
                    e.partial = {k: out[k][:F + (k == "out_off")] for k in ("changed", "count", "out_off")}
                raise e
            return {"changed": out["changed"][:F], "count": out["count"][:F], "out_off": out["out_off"][:F + 1],
                    "out_cluster": out["out_cluster"][:int(out["out_off"][F])], "calls": calls}

    def follower_timing(self):
        """kad_follower_timing: device ms of the last follower_union() — (the union / compare kernel, the offset
        scan + the emit kernel)."""
        return self._timing("follower", 2)

    def follower_last_route(self) -> dict:
        """kad_follower_last_route: what the last follower_union() launched (follower_route_eval's record)."""
        return _follower_route_dict(self._last_route("follower", FOLLOWER_ROUTE))

    def migrate_estimate(self, n_ids: int, now_ns: int, **arrays) -> dict:
        """kad_migrate_estimate → {uns[S], next_cross[S], cap[S], changed[O], n_written[O], retry_after[O],
        backoff[O]}. Arguments as :func:`migrate_args` (automigration.MigrationBatch.arrays())."""
        return self._consume("kad_migrate_estimate", migrate_args(n_ids, now_ns, **arrays))

    def migrate_timing(self):
        """kad_migrate_timing: device ms of the last migrate_estimate() — (migrate_segment_kernel,
        migrate_object_kernel)."""
        return self._timing("migrate", 2)

    def migrate_last_route(self) -> dict:
        """kad_migrate_last_route: what the last migrate_estimate() launched (migrate_route_eval's record)."""
        return self._last_route("migrate", MIGRATE_ROUTE)

    def migrate_debug_route(self, width: int = 0, long_min: int = 0) -> None:
        """kad_migrate_debug_route: the group width / long_min of the following migrate_estimate() calls
        (0: the route's own). Measurement only."""
        self._debug_route("migrate", width, long_min)

    def cluster_resources(self, n_res: int, **arrays) -> dict:
        """kad_cluster_resources → {alloc[K * R], avail[K * R], has[K], sched_nodes[K]}. Arguments as
        :func:`cstat_args` (clusterstatus.ClusterStatusBatch.arrays())."""
        return self._consume("kad_cluster_resources", cstat_args(n_res, **arrays))

    def cstat_timing(self):
        """kad_cstat_timing: device ms of the last cluster_resources() — (cstat_node_kernel, cstat_pod_kernel +
        cstat_combine_kernel)."""
        return self._timing("cstat", 2)

    def cstat_last_route(self) -> dict:
        """kad_cstat_last_route: what the last cluster_resources() launched (cstat_route_eval's record)."""
        return self._last_route("cstat", CSTAT_ROUTE)

    def cstat_debug_route(self, width: int = 0, long_min: int = 0) -> None:
        """kad_cstat_debug_route: the group width / long_min of the following cluster_resources() calls (0: the
        route's own). Measurement only."""
        self._debug_route("cstat", width, long_min)

    def status_aggregate(self, kind: int, **arrays) -> dict:
        """kad_status_aggregate → {sums[NV, O], changed[O]} and, Deployment, {observed[O]} or, Job, {start_min[O],
        done_max[O], n_done[O], n_failed[O], finished[O]}. Arguments as :func:`sagg_args`
        (statusagg.StatusAggBatch.arrays())."""
        return self._consume("kad_status_aggregate", sagg_args(kind, **arrays))

    def sagg_timing(self):
        """kad_sagg_timing: device ms of the last status_aggregate() — (sagg_kernel,)."""
        return self._timing("sagg", 1)

    def sagg_last_route(self) -> dict:
        """kad_sagg_last_route: what the last status_aggregate() launched (sagg_route_eval's record)."""
        return self._last_route("sagg", SAGG_ROUTE)

    def sagg_debug_route(self, width: int = 0, long_min: int = 0) -> None:
        """kad_sagg_debug_route: the group width / long_min of the following status_aggregate() calls (0: the
        route's own). Measurement only."""
        self._debug_route("sagg", width, long_min)

    def rollout_plan(self, **arrays) -> dict:
        """kad_rollout_plan → {replicas[T], max_surge[T], max_unavailable[T], plan_flags[T], action[T], status[O]}.
        Arguments as :func:`rollout_args` (rollout.RolloutBatch.arrays())."""
        return self._consume("kad_rollout_plan", rollout_args(**arrays))

    def rollout_timing(self):
        """kad_rollout_timing: device ms of the last rollout_plan() — (rollout_kernel,)."""
        return self._timing("rollout", 1)

    def rollout_last_route(self) -> dict:
        """kad_rollout_last_route: what the last rollout_plan() launched (rollout_route_eval's record)."""
        return self._last_route("rollout", ROLLOUT_ROUTE)

    def rollout_debug_route(self, width: int = 0, long_min: int = 0, serial: int = 0) -> None:
        """kad_rollout_debug_route: the group width / long_min of the following rollout_plan() calls (0: the
        route's own); serial = 1 walks every object serially. Measurement only."""
        self._debug_route("rollout", width, long_min, serial)

    def dispatch_plan(self, fill: int = 0, **arrays) -> dict:
        """kad_dispatch_plan → {out_cluster, out_op, out_status (object o's entries at out_off[o] .. + count[o]),
        count[O], n_ops[O], n_selected[O], obj_result[O]}. Arguments as :func:`dispatch_args`
        (dispatch.DispatchBatch.arrays()); the slots behind an object's entries keep ``fill``."""
        return self._consume("kad_dispatch_plan", dispatch_args(fill, **arrays))

    def dispatch_timing(self):
        """kad_dispatch_timing: ms of the last dispatch_plan() — (inputs to the device, dispatch_wave_kernel,
        outputs back)."""
        return self._timing("dispatch", 3)

    def dispatch_last_route(self) -> dict:
        """kad_dispatch_last_route: what the last dispatch_plan() launched (dispatch_route_eval's record)."""
        return self._last_route("dispatch", DISPATCH_ROUTE)

    def deletion_plan(self, fill: int = 0, pad: int = 0, **arrays) -> dict:
        """kad_deletion_plan → {out_op (aligned with the observations), n_ops[O], n_remaining[O],
        n_retrieval_failed[O], obj_pre[O], obj_first[O]}. Arguments as :func:`deletion_args`
        (deletion.DeletionBatch.arrays())."""
        return self._consume("kad_deletion_plan", deletion_args(fill, pad, **arrays))

    def deletion_finish(self, fill: int = 0, pad: int = 0, **arrays) -> dict:
        """kad_deletion_finish → {obj_status[O], obj_reason[O], obj_then[O], n_failed_ops[O], n_failed_checks[O]}.
        Arguments as :func:`deletion_finish_args` (deletion.DeletionBatch.finish_arrays())."""
        b, v, _keepalive, out, res = deletion_finish_args(fill, pad, **arrays)
        self._chk(self.L.kad_deletion_finish(self.h, ctypes.byref(b), ctypes.byref(res), ctypes.byref(v)))
        return out

    def deletion_timing(self):
        """kad_deletion_timing: ms of the last deletion_plan() — (inputs to the device, deletion_count_kernel +
        deletion_kernel, outputs back)."""
        return self._timing("deletion", 3)

    def deletion_finish_timing(self):
        """kad_deletion_finish_timing: ms of the last deletion_finish(), as :meth:`deletion_timing`."""
        return self._timing("deletion_finish", 3)

    def deletion_last_route(self) -> dict:
        """kad_deletion_last_route: what the last deletion_plan() launched (deletion_route_eval's record)."""
        return self._last_route("deletion", DELETION_ROUTE)

    def deletion_finish_last_route(self) -> dict:
        """kad_deletion_finish_last_route: what the last deletion_finish() launched."""
        return self._last_route("deletion_finish", DELETION_ROUTE)

    def deletion_debug_route(self, width: int = 0, long_min: int = 0) -> None:
        """kad_deletion_debug_route: the lane-group width and long_min of the following deletion_plan() calls (0:
        the route's own). Measurement and tests only."""
        self._debug_route("deletion", width, long_min)

    def deletion_finish_debug_route(self, width: int = 0, long_min: int = 0) -> None:
        """kad_deletion_finish_debug_route: as :meth:`deletion_debug_route`, for deletion_finish()."""
        self._debug_route("deletion_finish", width, long_min)

    def policyrc_count(self, **arrays) -> dict:
        """kad_policyrc_count → {new_count[P], new_total[P], state[P] (PRC_FLAGGED | PRC_UPDATE | PRC_NEGATIVE),
        n_negative[1]}. Arguments as :func:`policyrc_args` (policyrc.PolicyRefCounter.arrays())."""
        return self._consume("kad_policyrc_count", policyrc_args(**arrays))

    def policyrc_timing(self):
        """kad_policyrc_timing: ms of the last policyrc_count() — (inputs to the device, the zeroing and
        prc_count_kernel, prc_apply_kernel)."""
        return self._timing("policyrc", 3)

    def policyrc_last_route(self) -> dict:
        """kad_policyrc_last_route: what the last policyrc_count() launched (policyrc_route_eval's record)."""
        return self._last_route("policyrc", POLICYRC_ROUTE)

    def sync_needs_update(self, n_clusters: int, **arrays) -> dict:
        """kad_sync_needs_update → {needs_update[n_rows], recorded[n_rows]}. Arguments as
        :func:`sync_needs_update_args` (syncfin.SyncFinishBatch.needs_update_arrays())."""
        return self._consume("kad_sync_needs_update", sync_needs_update_args(n_clusters, **arrays))

    def sync_needs_update_timing(self):
        """kad_sync_needs_update_timing: ms of the last sync_needs_update() — (inputs to the device,
        syncfin_rows_kernel, outputs back)."""
        return self._timing("sync_needs_update", 3)

    def sync_needs_update_last_route(self) -> dict:
        """kad_sync_needs_update_last_route: what the last sync_needs_update() launched."""
        return self._last_route("sync_needs_update", SYNC_NU_ROUTE)

    def sync_finish(self, n_clusters: int, n_reasons: int, reason_check_clusters: int, reason_ns_not_federated: int,
                    **arrays) -> dict:
        """kad_sync_finish → {out_ver_cluster, out_ver_id (object o's entries at ver_off[o] .. + ver_count[o]),
        ver_count[O], ver_write[O], out_st_cluster, out_st_status, out_st_gen (at st_off[o] .. + st_count[o]),
        st_count[O], obj_out[O], reason_out[O]}. Arguments as :func:`sync_finish_args`
        (syncfin.SyncFinishBatch.finish_arrays())."""
        return self._consume("kad_sync_finish", sync_finish_args(n_clusters, n_reasons, reason_check_clusters,
                                                                 reason_ns_not_federated, **arrays))

    def sync_finish_timing(self):
        """kad_sync_finish_timing: ms of the last sync_finish() — (inputs to the device, syncfin_kernel, outputs
        back)."""
        return self._timing("sync_finish", 3)

    def sync_finish_last_route(self) -> dict:
        """kad_sync_finish_last_route: what the last sync_finish() launched (sync_finish_route_eval's record)."""
        return self._last_route("sync_finish", SYNC_FIN_ROUTE)

    def revision_plan(self, n_pairs: int, **arrays) -> dict:
        """kad_revision_plan → {out_off[O + 1], hash[O], upd_hash[O], upd_parsed[O], equal[R], order[R] (object o's
        sorted old revisions at rev_off[o] .. + n_old[o]), n_old[O], keep[O], n_actions[O], last[O], rev_number[O],
        act_kind / act_rev (object o's actions at out_off[o] .. + n_actions[o])}. Arguments as
        :func:`revision_plan_args` (history.RevisionBatch.arrays())."""
        return self._consume("kad_revision_plan", revision_plan_args(n_pairs, **arrays))

    def revision_plan_timing(self):
        """kad_revision_plan_timing: ms of the last revision_plan() — (hr_hash_kernel, hr_compare_kernel,
        hr_plan_kernel)."""
        return self._timing("revision_plan", 3)

    def revision_plan_last_route(self) -> dict:
        """kad_revision_plan_last_route: what the last revision_plan() launched (revision_plan_route_eval's record)."""
        return self._last_route("revision_plan", REVISION_ROUTE)

    def revision_plan_debug_route(self, width: int = 0, long_min: int = 0) -> None:
        """kad_revision_plan_debug_route: the lane-group width of the compare and the plan kernel and long_min of the
        following revision_plan() calls (0: the route's own)."""
        self._debug_route("revision_plan", width, long_min)

    def sync_finish_debug_route(self, width: int = 0, long_min: int = 0) -> None:
        """kad_sync_finish_debug_route: the lane-group width and long_min of the following sync_finish() calls (0:
        the route's own). Measurement and tests only."""
        self._debug_route("sync_finish", width, long_min)

    # ---- the monitor's resident meter table (kad_monitor_*)
    def monitor_reserve(self, capacity: int) -> None:
        """kad_monitor_reserve: the meter table holds at least ``capacity`` slots; its contents stay."""
        self._chk(self.L.kad_monitor_reserve(self.h, int(capacity)))

    def monitor_info(self) -> dict:
        """kad_monitor_info: the table's capacity, n_slots (what a report walks), live slots and highest type id."""
        out = (ctypes.c_int64 * 4)()
        self._chk(self.L.kad_monitor_info(self.h, out))
        return dict(zip(("capacity", "n_slots", "n_live", "max_type"), (int(x) for x in out)))

    def monitor_load(self, slots, type_id=None, flags=None, **columns) -> None:
        """kad_monitor_load: writes the listed slots' given columns (MONITOR_COLUMNS by name, int64 ns), type ids
        and flags (KAD_MON_LIVE); a column left out keeps its contents."""
        sl = np.ascontiguousarray(slots, np.int32).reshape(-1)
        bad = set(columns) - set(MONITOR_COLUMNS)
        if bad:
            raise TypeError(f"unknown monitor columns {sorted(bad)}")
        cols = [None if k not in columns else np.ascontiguousarray(columns[k], np.int64).reshape(-1) for k in MONITOR_COLUMNS]
        ty = None if type_id is None else np.ascontiguousarray(type_id, np.int32).reshape(-1)
        fl = None if flags is None else np.ascontiguousarray(flags, np.uint8).reshape(-1)
        for a in cols + [ty, fl]:
            if a is not None and len(a) != len(sl):
                raise ValueError("monitor_load: a column's length differs from the slots'")
        self._chk(self.L.kad_monitor_load(self.h, len(sl), _p(sl), *(_p(a) for a in cols), _p(ty), _p(fl)))

    def monitor_read(self, slots) -> dict:
        """kad_monitor_read → the listed slots' MONITOR_COLUMNS, ``type_id`` and ``flags``."""
        sl = np.ascontiguousarray(slots, np.int32).reshape(-1)
        n = max(1, len(sl))
        out = {k: np.zeros(n, np.int64) for k in MONITOR_COLUMNS}
        out["type_id"] = np.zeros(n, np.int32)
        out["flags"] = np.zeros(n, np.uint8)
        self._chk(self.L.kad_monitor_read(self.h, len(sl), _p(sl), *(_p(a) for a in out.values())))
        return {k: v[:len(sl)] for k, v in out.items()}

    def monitor_clear(self) -> None:
        """kad_monitor_clear: no slot is live; the capacity stays."""
        self._chk(self.L.kad_monitor_clear(self.h))

    def monitor_reconcile(self, n_clusters: int, now_ns: int, **arrays) -> dict:
        """kad_monitor_reconcile → {result[O], bits[O], meter[O, 5], would[O, 2]}. Arguments as
        :func:`monitor_reconcile_args` (monitor.MonitorBatch.arrays())."""
        out = self._consume("kad_monitor_reconcile", monitor_reconcile_args(n_clusters, now_ns, **arrays))
        out["meter"] = out["meter"].reshape(-1, 5)
        out["would"] = out["would"].reshape(-1, 2)
        return out

    def monitor_report(self, now_ns: int, n_types: int, timer_cap: Optional[int] = None) -> dict:
        """kad_monitor_report → {counters[14], type_sync[n_types], type_status[n_types], sync_slot / sync_ms and
        status_slot / status_ms cut to their lengths, n_timers[2]}. ``timer_cap`` defaults to the longer list of
        this context's last report plus a quarter (1024 at least), so that a steady table is walked once; a list
        that is longer all the same is fetched again with room for it."""
        if timer_cap is None:
            timer_cap = max(1024, getattr(self, "_monitor_timer_cap", 0))
        while True:
            args = monitor_report_args(now_ns, n_types, timer_cap)
            b, v, _, out = args
            rc = self.L.kad_monitor_report(self.h, ctypes.byref(b), ctypes.byref(v))
            need = int(out["n_timers"].max())
            if rc == KAD_ENOSPC and need > timer_cap:
                timer_cap = need
                continue
            self._chk(rc)
            self._monitor_timer_cap = need + need // 4
            ns, nt = (int(x) for x in out["n_timers"])
            for k in ("sync_slot", "sync_ms"):
                out[k] = out[k][:ns]
            for k in ("status_slot", "status_ms"):
                out[k] = out[k][:nt]
            return out

    def monitor_reconcile_timing(self):
        """kad_monitor_reconcile_timing: ms of the last monitor_reconcile() (inputs in, the kernel, outputs back)."""
        return self._timing("monitor_reconcile", 3)

    def monitor_report_timing(self):
        """kad_monitor_report_timing: ms of the last monitor_report() (the zeroing, monitor_scan_kernel, the
        offsets and monitor_scatter_kernel)."""
        return self._timing("monitor_report", 3)

    def monitor_reconcile_last_route(self) -> dict:
        """kad_monitor_reconcile_last_route: what the last monitor_reconcile() launched."""
        return self._last_route("monitor_reconcile", MONITOR_REC_ROUTE)

    def monitor_report_last_route(self) -> dict:
        """kad_monitor_report_last_route: what the last monitor_report() launched."""
        return self._last_route("monitor_report", MONITOR_REP_ROUTE)

    def monitor_reconcile_debug_route(self, width: int = 0, long_min: int = 0) -> None:
        """kad_monitor_reconcile_debug_route: the lane-group width and long_min of the following calls (0: the
        route's own)."""
        self._debug_route("monitor_reconcile", width, long_min)

    def monitor_report_debug_route(self, path: int = 0, grid: int = 0) -> None:
        """kad_monitor_report_debug_route: the histogram path (1 LDS-private, 2 global) and the blocks of the
        following reports (0: the route's own)."""
        self._debug_route("monitor_report", path, grid)

    def policyrc_debug_route(self, path: int = 0) -> None:
        """kad_policyrc_debug_route: the count kernel's path of the following policyrc_count() calls (0: the
        route's own, 1: LDS-private, 2: global)."""
        self._debug_route("policyrc", path)

    def select_rows(self, rows: Sequence[Sequence[int]], max_clusters: Sequence[Optional[int]], flags: int = 0):
        """MaxCluster on explicit score rows → per row (status, sorted selected positions)."""
        off = np.zeros(len(rows) + 1, np.int32)
        off[1:] = np.cumsum([len(r) for r in rows])
        scores = np.array([x for r in rows for x in r] or [0], np.int64)
        mc = np.array([(np.iinfo(np.int64).max if m is None else m) for m in max_clusters], np.int64)
        cnt = np.zeros(len(rows), np.int32)
        st = np.zeros(len(rows), np.int32)
        sel = np.zeros(max(1, int(off[-1])), np.int32)
        self._chk(self.L.kad_select_rows(self.h, len(rows), _p(off), _p(scores), _p(mc), flags, _p(cnt), _p(sel),
                                         _p(st)))
        return [(int(st[r]), sel[off[r]:off[r] + cnt[r]].tolist()) for r in range(len(rows))]

    def plan_rows(self, rows):
        """planner.Plan on explicit rows.

        rows: list of dicts with ``elems`` (list of dicts hash, weight, min, max(None), cap(None), current),
        ``total``, ``avoid``, ``keep``. Returns per row (plan list, overflow list with None for absent).
        """
        n = len(rows)
        off = np.zeros(n + 1, np.int32)
        off[1:] = np.cumsum([len(r["elems"]) for r in rows])
        tot = max(1, int(off[-1]))
        hsh = np.zeros(tot, np.uint32)
        wt, mn, mx, cp, cur = (np.zeros(tot, np.int64) for _ in range(5))
        ef = np.zeros(tot, np.uint32)
        i = 0
        for r in rows:
            for e in r["elems"]:
                hsh[i], wt[i], mn[i], cur[i] = e["hash"], e["weight"], e["min"], e["current"]
                if e.get("max") is not None:
                    mx[i] = e["max"]
                    ef[i] |= 2
                if e.get("cap") is not None:
                    cp[i] = e["cap"]
                    ef[i] |= 4
                i += 1
        total = np.array([r["total"] for r in rows] or [0], np.int64)
        rf = np.array([(1 if r["avoid"] else 0) | (2 if r["keep"] else 0) for r in rows] or [0], np.uint32)
        plan = np.zeros(tot, np.int64)
        over = np.zeros(tot, np.int64)
        self._chk(self.L.kad_plan_rows(self.h, n, _p(off), _p(hsh), _p(wt), _p(mn), _p(mx), _p(cp), _p(cur), _p(ef),
                                       _p(total), _p(rf), _p(plan), _p(over)))
        out = []
        for r in range(n):
            a, b = off[r], off[r + 1]
            out.append((plan[a:b].tolist(), [None if o < 0 else int(o) for o in over[a:b].tolist()]))
        return out


    # ------------------------------------------------ scheduling-trigger hashes
    def trigger_suffix_upload(self, suffix: bytes):
        buf = np.frombuffer(suffix, np.uint8) if suffix else np.zeros(1, np.uint8)
        self._chk(self.L.kad_trigger_suffix_upload(self.h, _p(buf), len(suffix)))

    def trigger_prefixes_upload(self, prefixes: Sequence[bytes]):
        off = np.zeros(len(prefixes) + 1, np.int64)
        off[1:] = np.cumsum([len(p) for p in prefixes])
        data = np.frombuffer(b"".join(prefixes) or b"\0", np.uint8)
        self._chk(self.L.kad_trigger_prefixes_upload(self.h, len(prefixes), _p(off), _p(data)))
        self._trig_n = len(prefixes)

    def trigger_run(self):
        self._chk(self.L.kad_trigger_run(self.h))

    def trigger_timing(self):
        return self._timing("trigger", 2)

    def trigger_download(self) -> np.ndarray:
        out = np.zeros(max(1, self._trig_n), np.uint32)
        self._chk(self.L.kad_trigger_download(self.h, _p(out)))
        return out[:self._trig_n]


def batch_split(batch, n: int):
    """kad_batch_split (host only): the contiguous unit ranges a kad_group of n members gives its members,
    and their first output slots: (unit_lo[n+1], slot_lo[n+1])."""
    L = load_library()
    ulo = np.zeros(n + 1, np.int64)
    slo = np.zeros(n + 1, np.int64)
    rc = L.kad_batch_split(_p(batch.blob), batch.blob.nbytes, n, _p(ulo), _p(slo))
    if rc != 0:
        raise KadError(rc, "kad_batch_split: malformed batch blob or n < 1")
    return ulo, slo


class _MemberContext(Context):
    """A kad_group member's kad_ctx, owned by the group (GroupContext.member)."""

    def close(self):
        self.h = None


class GroupContext:
    """A kad_group: one process scheduling each batch over several GPUs (contiguous unit ranges, one
    kad_ctx per device), results in one view as from a single Context. Same interface as :class:`Context`
    for what :class:`BatchScheduler` uses (upload_snapshot, update_snapshot, upload_batch, schedule, sync,
    download, run, path_counts), so a BatchScheduler / CoalescingScheduler drives N GPUs unchanged."""

    def __init__(self, devices: Sequence[int]):
        self.devices = list(devices)
        self.L = load_library()
        h = ctypes.c_void_p()
        arr = (ctypes.c_int * len(self.devices))(*self.devices)
        rc = self.L.kad_group_create(arr, len(self.devices), ctypes.byref(h))
        if rc != 0:
            raise KadError(rc, f"kad_group_create(devices={self.devices}) failed (no GPU?)")
        self.h = h
        self.snap: Optional[Snapshot] = None
        self.batch: Optional[Batch] = None

    @property
    def device(self):
        return self.devices[0]

    def close(self):
        if self.h:
            self.L.kad_group_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _chk(self, rc):
        if rc != 0:
            raise KadError(rc, self.L.kad_group_last_error(self.h).decode())

    def upload_snapshot(self, snap: Snapshot):
        self._chk(self.L.kad_group_snapshot_upload(self.h, _p(snap.blob), snap.blob.nbytes))
        self.snap = snap

    def member(self, i: int) -> "Context":
        """kad_group_member: member i's kad_ctx (its shard of the resident batch) as a Context that the group
        owns (closing it does nothing). Its per-ctx calls — copy_results_device, result_diff, path_counts,
        stage_timing — cover the member's units."""
        c = ctypes.c_void_p()
        self._chk(self.L.kad_group_member(self.h, i, ctypes.byref(c)))
        m = _MemberContext.__new__(_MemberContext)
        m.device, m.L, m.h, m.snap, m.batch = self.devices[i], self.L, c, self.snap, None
        return m

    def update_snapshot(self, delta: SnapshotDelta):
        self._chk(self.L.kad_group_snapshot_update(self.h, _p(delta.blob), delta.blob.nbytes))

    def upload_batch(self, batch: Batch):
        chk = getattr(batch, "check_current", None)
        if chk is not None:
            chk()
        self._chk(self.L.kad_group_batch_upload(self.h, _p(batch.blob), batch.blob.nbytes))
        self.batch = batch

    def schedule(self, fwk: Framework):
        prof = fwk.to_c()
        self._chk(self.L.kad_group_schedule(self.h, ctypes.byref(prof)))

    def sync(self):
        self._chk(self.L.kad_group_sync(self.h))

    def set_timing(self, on: bool):
        self._chk(self.L.kad_group_set_timing(self.h, 1 if on else 0))

    def ranges(self):
        n = len(self.devices)
        ulo = np.zeros(n + 1, np.int64)
        slo = np.zeros(n + 1, np.int64)
        self._chk(self.L.kad_group_ranges(self.h, _p(ulo), _p(slo)))
        return ulo, slo

    def path_counts(self) -> dict:
        out = (ctypes.c_int32 * 4)()
        self._chk(self.L.kad_group_path_counts(self.h, out))
        return {"units": out[0], "full_kernel": out[1], "row_kernel": out[2], "planner_rows": out[3]}

    def member_stage_timing(self, i: int) -> dict:
        """kad_stage_timing of member i (timing on)."""
        c = ctypes.c_void_p()
        self._chk(self.L.kad_group_member(self.h, i, ctypes.byref(c)))
        ms = (ctypes.c_float * 7)()
        rc = self.L.kad_stage_timing(c, ms, 7)
        if rc != 0:
            raise KadError(rc, self.L.kad_last_error(c).decode())
        return {k: float(v) for k, v in zip(Context.STAGES, ms)}

    def download(self, out: Optional[BatchResult] = None) -> BatchResult:
        res = BatchResult.empty(self.batch) if out is None else out
        v = ResultView(res.status.ctypes.data, res.count.ctypes.data, res.flags.ctypes.data, res.cluster.ctypes.data,
                       res.replicas.ctypes.data)
        self._chk(self.L.kad_group_results_download(self.h, ctypes.byref(v)))
        return res

    def schedule_batch(self, fwk: Framework, batch: Batch) -> BatchResult:
        res = BatchResult.empty(batch)
        v = ResultView(res.status.ctypes.data, res.count.ctypes.data, res.flags.ctypes.data, res.cluster.ctypes.data,
                       res.replicas.ctypes.data)
        prof = fwk.to_c()
        self._chk(self.L.kad_group_schedule_batch(self.h, ctypes.byref(prof), _p(batch.blob), batch.blob.nbytes,
                                                  ctypes.byref(v)))
        self.batch = batch
        return res

    def run(self, fwk: Framework, batch: Batch) -> BatchResult:
        self.upload_batch(batch)
        self.schedule(fwk)
        return self.download()


class TriggerHasher:
    """Scheduler.computeSchedulingTriggerHash for a batch of objects (schedulingtriggers.go:106-147).

    The cluster part of the trigger JSON is built once per cluster list
    (:meth:`set_clusters`), each object's part on the host, and the FNV-1 over
    object part ‖ cluster part runs on the GPU (``kad_trigger_*``). Returns the
    decimal strings the reference writes to the
    ``kubeadmiral.io/scheduling-trigger-hash`` annotation.
    """

    def __init__(self, ctx: Optional[Context] = None, device: int = 0):
        self.ctx = ctx if ctx is not None else Context(device)
        self.suffix: Optional[bytes] = None

    def set_clusters(self, clusters: List[T.FederatedCluster]) -> bytes:
        from .objects import trigger_suffix

        self.suffix = trigger_suffix(clusters)
        self.ctx.trigger_suffix_upload(self.suffix)
        return self.suffix

    def hashes(self, type_config, objs: Sequence[dict], policies: Sequence) -> List[str]:
        from .objects import format_trigger_hash, trigger_prefix

        if self.suffix is None:
            raise RuntimeError("set_clusters first")
        self.ctx.trigger_prefixes_upload([trigger_prefix(type_config, o, p) for o, p in zip(objs, policies)])
        self.ctx.trigger_run()
        h = self.ctx.trigger_download()
        return [format_trigger_hash(x) for x in h.tolist()]


class BatchScheduler:
    """Batch ScheduleAlgorithm on the GPU (generic_scheduler.go:37-44 semantics per unit).

    The resident snapshot follows the cluster list of every call: each call
    diffs the list against it by content (``types.cluster_key``), so a new
    list, replaced elements or elements edited in place are all picked up —
    the library keeps no caller pointers. Host columns are committed only
    after the device accepted the delta; a failed device update forces a full
    re-upload on the next call.
    """

    def __init__(self, ctx: Optional[Context] = None, device: int = 0, devices: Optional[Sequence[int]] = None):
        """``devices``: schedule every batch over these GPUs (a :class:`GroupContext`, one process), else one
        Context on ``device``."""
        if ctx is None:
            ctx = GroupContext(devices) if devices is not None else Context(device)
        self.ctx = ctx
        self.full_uploads = 0   # snapshot (re)packs + uploads
        self.delta_updates = 0  # in-place kad_snapshot_update calls

    def set_clusters(self, clusters: List[T.FederatedCluster]) -> Snapshot:
        """Make ``clusters`` the resident snapshot: an in-place delta when only existing clusters changed
        within the interned vocabulary (cluster status / label / taint events, scheduler.go:157-177), else a
        repack and full upload (join, leave, new label value / taint / API resource)."""
        snap = self.ctx.snap
        if snap is not None:
            delta = snap.diff(clusters)
            if delta is not None:
                if delta.changed:
                    try:
                        self.ctx.update_snapshot(delta)
                    except BaseException:
                        self.ctx.snap = None  # device state unknown: the next call re-uploads in full
                        raise
                    self.delta_updates += 1
                snap.commit(delta)
                return snap
        snap = Snapshot(clusters)
        self.ctx.upload_snapshot(snap)
        self.full_uploads += 1
        return snap

    def schedule(self, fwk: Framework, units: List[T.SchedulingUnit], clusters: List[T.FederatedCluster]
                 ) -> List[Union[T.ScheduleResult, T.ScheduleError]]:
        snap = self.set_clusters(clusters)
        batch = Batch(snap, fwk, units)
        res = self.ctx.run(fwk, batch)
        return [to_schedule_result(res, w, su, snap.names) for w, su in enumerate(units)]

    def schedule_columns(self, fwk: Framework, cols, clusters: List[T.FederatedCluster]):
        """The same for units already in columns (``columns.SUColumns``, e.g. from ``columns.units_from_objects``):
        the native packer, one GPU batch. Returns (BatchResult, snapshot)."""
        from .columns import NativePacker

        snap = self.set_clusters(clusters)
        pk = getattr(self, "_packer", None)
        if pk is None or pk.snap is not snap or getattr(self, "_packer_fp", None) != snap.fingerprint:
            pk = self._packer = NativePacker(snap)  # the packer interns against the snapshot's vocabulary
            self._packer_fp = snap.fingerprint
        batch = pk.pack(fwk, cols)
        return self.ctx.run(fwk, batch), snap
