// Rollout planning (kad_rollout_plan): for every member cluster of a federated Deployment that is rolling out, the
// replicas, maxSurge and maxUnavailable it may be given now, so that the federation as a whole stays inside the
// template's own maxSurge / maxUnavailable, and the dispatch operation that follows.
//
// RolloutPlanner.Plan (pkg/controllers/util/rolloutplan.go:569-695) walks an object's targets, sorted by cluster
// name, five times and carries two budgets (the remaining maxSurge and maxUnavailable) along. Every other term
// depends on the target alone. In each pass a target takes min(budget, its offer) from a positive budget and
// nothing from one that is not, so a budget after some targets is m0 if m0 <= 0 and max(m0 - sum of their offers,
// 0) otherwise: each pass is an exclusive prefix sum of the offers over the sorted order and a per-lane evaluation.
//
//   rollout_kernel<W>  blocks below long_grid: four waves, each one listed long object; the other blocks: a wave is
//                      64 / W lane groups, each group plans one object at a time, a target per lane, in chunks of
//                      W with the prefix sums carried from chunk to chunk
//
// The prefix-sum form needs arithmetic that does not wrap; the host marks the objects where it could (obj_mode
// RO_MODE_SERIAL) and one lane of the group walks those as the reference does, in wrapping arithmetic
// (ro_serial, which is also what the prefix-sum form is tested against). No LDS, no atomics, no state that
// kad_schedule reads.
#include "kad_rollout.h"
#include "kad_wave.h"

namespace kad {

KAD_HD RoTarget ro_load(const RolloutDev& d, int64_t i) {
  RoTarget t;
  const int64_t T = d.T;
  t.r = d.tgt_vals[RO_REPLICAS * T + i];
  t.act = d.tgt_vals[RO_ACTUAL * T + i];
  t.av = d.tgt_vals[RO_AVAILABLE * T + i];
  t.ur = d.tgt_vals[RO_UPDATED * T + i];
  t.uar = d.tgt_vals[RO_UPDATED_AVAILABLE * T + i];
  t.cn = d.tgt_vals[RO_CURRENT_NEW * T + i];
  t.cna = d.tgt_vals[RO_CURRENT_NEW_AVAILABLE * T + i];
  t.ms = d.tgt_vals[RO_MAX_SURGE * T + i];
  t.mu = d.tgt_vals[RO_MAX_UNAVAILABLE * T + i];
  t.d = d.tgt_vals[RO_DESIRED * T + i];
  t.f = d.tgt_flags[i];
  ro_derive(t);
  return t;
}
KAD_HD void ro_store(const RolloutDev& d, int64_t i, uint8_t tf, const RoPlan& p) {
  d.replicas[i] = (p.f & RO_HAS_REPLICAS) ? p.r : 0;
  d.max_surge[i] = (p.f & RO_HAS_SURGE) ? p.s : 0;
  d.max_unavailable[i] = (p.f & RO_HAS_UNAVAILABLE) ? p.u : 0;
  d.plan_flags[i] = p.f;
  d.action[i] = ro_action(tf, p);
}
KAD_HD RoPlan ro_load_plan(const RolloutDev& d, int64_t i) {
  return RoPlan{d.replicas[i], d.max_surge[i], d.max_unavailable[i], d.plan_flags[i]};
}
// no target of [lo, hi) planned
KAD_HD void ro_store_unplanned(const RolloutDev& d, int64_t lo, int64_t hi, int first, int step) {
  for (int64_t i = lo + first; i < hi; i += step) ro_store(d, i, d.tgt_flags[i], RoPlan{0, 0, 0, 0});
}

// Plan() as the reference walks it, one object on one thread, in Go's wrapping int32. The plans under way live
// in the output arrays (pass 4 reads pass 1's, pass 5 reads pass 2's).
KAD_HD void ro_serial(const RolloutDev& d, int o) {
  const int64_t lo = d.obj_tgt_off[o], hi = d.obj_tgt_off[o + 1];
  const int32_t p_ms = d.obj_max_surge[o], p_mu = d.obj_max_unavailable[o], p_rep = d.obj_replicas[o];
  const bool p_surge = p_ms != 0 && p_mu == 0;
  int32_t sum_r = 0, occ_s = 0, occ_u = 0, desired = 0;
  bool any_out = false, any_in = false, settled = true;
  for (int64_t i = lo; i < hi; ++i) {
    const RoTarget t = ro_load(d, i);
    sum_r = ro_add(sum_r, t.r);
    occ_s = ro_add(occ_s, t.ls);
    occ_u = ro_add(occ_u, t.lu);
    desired = ro_add(desired, t.d);
    any_out |= t.cls == RO_CLS_OUT;
    any_in |= t.cls == RO_CLS_IN;
    settled &= t.completed && !ro_flip(t, p_surge);
  }
  if (any_out != any_in && settled) {  // IsScalingEvent (:502-520) → PlanScale
    for (int64_t i = lo; i < hi; ++i) ro_store(d, i, d.tgt_flags[i], RoPlan{0, 0, 0, RO_PLANNED});
    d.status[o] = RO_SCALE;
    return;
  }
  int32_t S = ro_sub(ro_sub(p_ms, ro_sub(sum_r, p_rep)), occ_s);  // RemainingMaxSurge (:539-548)
  int32_t U = ro_sub(ro_sub(p_mu, ro_sub(p_rep, sum_r)), occ_u);  // RemainingMaxUnavailable (:550-559)
  ro_store_unplanned(d, lo, hi, 0, 1);
  int32_t sm, um;
  for (int64_t i = lo; i < hi; ++i) {  // 1. upgrade targets waiting to be scaled out
    const RoTarget t = ro_load(d, i);
    if (t.cls != RO_CLS_OUT || ro_skip_update(t, S, U)) continue;
    RoPlan p{t.r, 0, 0, RO_HAS_REPLICAS};
    ro_fenceposts(t, S, U, t.lu, p_surge, p, sm, um);
    S = ro_sub(S, sm);
    U = ro_sub(U, um);
    ro_store(d, i, t.f, p);
  }
  for (int64_t i = lo; i < hi; ++i) {  // 2. scale in targets waiting to be scaled in
    const RoTarget t = ro_load(d, i);
    if (t.cls != RO_CLS_IN || (U <= 0 && t.lu <= 0)) continue;
    const RoFence f = ro_scale_in(U, t.during ? 0 : t.lu, t);
    U = ro_sub(U, f.more);
    ro_store(d, i, t.f, RoPlan{ro_sub(t.r, f.res), 0, 0, RO_PLANNED | RO_HAS_REPLICAS | RO_ONLY_PATCH_REPLICAS});
  }
  for (int64_t i = lo; i < hi; ++i) {  // 3. upgrade targets that only need to be upgraded
    const RoTarget t = ro_load(d, i);
    if (t.cls != RO_CLS_UPDATE || ro_skip_update(t, S, U)) continue;
    RoPlan p{0, 0, 0, 0};
    ro_fenceposts(t, S, U, t.lu, p_surge, p, sm, um);
    S = ro_sub(S, sm);
    U = ro_sub(U, um);
    ro_store(d, i, t.f, p);
  }
  for (int64_t i = lo; i < hi; ++i) {  // 4. scale out targets waiting to be scaled out
    const RoTarget t = ro_load(d, i);
    if (t.cls != RO_CLS_OUT || (S <= 0 && t.ls <= 0)) continue;
    if (!t.upd && t.r != 0) continue;  // the new replica set must exist
    const RoFence f = ro_scale_out(S, t.during ? 0 : t.ls, t);
    S = ro_sub(S, f.more);
    RoPlan p = ro_load_plan(d, i);
    p.r = ro_add(t.r, f.res);
    p.f |= RO_PLANNED | RO_HAS_REPLICAS;
    ro_store(d, i, t.f, p);
  }
  for (int64_t i = lo; i < hi; ++i) {  // 5. upgrade targets waiting to be scaled in
    const RoTarget t = ro_load(d, i);
    if (t.cls != RO_CLS_IN) continue;
    RoPlan p = ro_load_plan(d, i);
    if (!(p.f & RO_PLANNED)) p = RoPlan{t.r, 0, 0, RO_HAS_REPLICAS};
    const int32_t lu5 = ro_lu5(t, p.r);
    if (ro_skip5(t, S, U, lu5)) continue;
    p.f &= (uint8_t)~RO_ONLY_PATCH_REPLICAS;
    ro_fenceposts(t, S, U, lu5, p_surge, p, sm, um);
    S = ro_sub(S, sm);
    U = ro_sub(U, um);
    ro_store(d, i, t.f, p);
  }
  int32_t planned = 0;
  for (int64_t i = lo; i < hi; ++i) planned = ro_add(planned, ro_planned_replicas(ro_load(d, i), ro_load_plan(d, i)));
  const bool invalid = ro_invalid(p_rep, p_ms, p_mu, planned, desired, sum_r);
  if (invalid) ro_store_unplanned(d, lo, hi, 0, 1);
  d.status[o] = invalid ? RO_INVALID : RO_OK;
}

// inclusive prefix sum within groups of W lanes: row shifts, masked below 16 lanes, then the row broadcasts
template <int W>
__device__ __forceinline__ int ro_scan(int v, int gl) {
  if (W >= 2) {
    const int t = dpp32<0x111, 0xf>(0, v);
    v += (W >= 16 || gl >= 1) ? t : 0;
  }
  if (W >= 4) {
    const int t = dpp32<0x112, 0xf>(0, v);
    v += (W >= 16 || gl >= 2) ? t : 0;
  }
  if (W >= 8) {
    const int t = dpp32<0x114, 0xf>(0, v);
    v += (W >= 16 || gl >= 4) ? t : 0;
  }
  if (W >= 16) v += dpp32<0x118, 0xf>(0, v);
  if (W >= 32) v += dpp32<0x142, 0xa>(0, v);
  if (W >= 64) v += dpp32<0x143, 0xc>(0, v);
  return v;
}
template <int W>
__device__ __forceinline__ int ro_group_sum(int v) {  // wrapping, to every lane of the group
#pragma unroll
  for (int m = W / 2; m >= 1; m >>= 1) v = (int)((uint32_t)v + (uint32_t)__shfl_xor(v, m));
  return v;
}
// exclusive prefix of offer a over the object's targets so far; carry takes the chunk's total
template <int W>
__device__ __forceinline__ int ro_prefix(int a, int gl, int& carry) {
  const int incl = ro_scan<W>(a, gl);
  const int x = carry + incl - a;
  carry += __shfl(incl, W - 1, W);
  return x;
}

enum { RO_A1S, RO_A1U, RO_A2U, RO_A3S, RO_A3U, RO_A4S, RO_NA };
// what a target offers to take in passes 1 to 4 (pass 5's offer to the unavailable budget depends on pass 2)
__device__ __forceinline__ void ro_offers(const RoTarget& t, int32_t a[RO_NA]) {
#pragma unroll
  for (int k = 0; k < RO_NA; ++k) a[k] = 0;
  if (t.cls == RO_CLS_OUT) {
    a[RO_A1S] = ro_offer(t.rtu, t.ls);
    a[RO_A1U] = ro_offer(t.rtua, t.lu);
    if (t.upd || t.r == 0) a[RO_A4S] = ro_offer(ro_sub(t.d, t.r), t.during ? 0 : t.ls);
  } else if (t.cls == RO_CLS_IN) {
    int32_t x = ro_sub(t.r, t.d);
    if (x > t.r) x = t.r;
    a[RO_A2U] = ro_offer(x, t.during ? 0 : t.lu);
  } else {
    a[RO_A3S] = ro_offer(t.rtu, t.ls);
    a[RO_A3U] = ro_offer(t.rtua, t.lu);
  }
}

// One object (o < 0: none) by the W lanes of a group, gl the lane's index in it. Every lane of the wave comes
// here together and the loops that scan run the same number of times on all of them.
template <int W>
__device__ __forceinline__ void plan_group(const RolloutDev& d, int o, int gl) {
  int64_t lo = 0;
  int n = 0;
  uint8_t of = 0, mode = 0;
  int32_t p_ms = 0, p_mu = 0, p_rep = 0;
  if (o >= 0) {
    lo = d.obj_tgt_off[o];
    n = d.obj_tgt_off[o + 1] - (int32_t)lo;
    of = d.obj_flags[o];
    mode = d.obj_mode[o];
    p_ms = d.obj_max_surge[o];
    p_mu = d.obj_max_unavailable[o];
    p_rep = d.obj_replicas[o];
  }
  const bool err = (of & RO_OBJ_ERROR) != 0, serial = o >= 0 && !err && (mode & RO_MODE_SERIAL);
  const int ns = (o >= 0 && !err && !serial) ? n : 0;  // the targets this group scans
  const bool p_surge = p_ms != 0 && p_mu == 0;
  if (err) {  // passed through: nothing planned (managed.go:215-235 goes on without plans)
    ro_store_unplanned(d, lo, lo + n, gl, W);
    if (gl == 0) d.status[o] = RO_ERROR;
  }
  if (serial && gl == 0) ro_serial(d, o);

  // ---- the sums over the object: the budgets' start, IsScalingEvent, each pass's total offer
  RoTarget t{};
  int32_t a[RO_NA];
  int32_t sum_r = 0, occ_s = 0, occ_u = 0, desired = 0, n_out = 0, n_in = 0, n_open = 0;
  int32_t tot[RO_NA] = {0, 0, 0, 0, 0, 0};
  for (int i = gl; i < ns; i += W) {
    t = ro_load(d, lo + i);
    ro_offers(t, a);
    sum_r = ro_add(sum_r, t.r);
    occ_s = ro_add(occ_s, t.ls);
    occ_u = ro_add(occ_u, t.lu);
    desired = ro_add(desired, t.d);
    n_out += t.cls == RO_CLS_OUT;
    n_in += t.cls == RO_CLS_IN;
    n_open += !(t.completed && !ro_flip(t, p_surge));
#pragma unroll
    for (int k = 0; k < RO_NA; ++k) tot[k] += a[k];
  }
  if (W > 1) {
    sum_r = ro_group_sum<W>(sum_r);
    occ_s = ro_group_sum<W>(occ_s);
    occ_u = ro_group_sum<W>(occ_u);
    desired = ro_group_sum<W>(desired);
    n_out = ro_group_sum<W>(n_out);
    n_in = ro_group_sum<W>(n_in);
    n_open = ro_group_sum<W>(n_open);
#pragma unroll
    for (int k = 0; k < RO_NA; ++k) tot[k] = ro_group_sum<W>(tot[k]);
  }
  const bool scaling = ((n_out != 0) != (n_in != 0)) && n_open == 0;
  const int32_t S0 = ro_sub(ro_sub(p_ms, ro_sub(sum_r, p_rep)), occ_s), U0 = ro_sub(ro_sub(p_mu, ro_sub(p_rep, sum_r)), occ_u);
  const int64_t T1s = tot[RO_A1S], T1u = tot[RO_A1U], T2u = tot[RO_A2U], T3s = tot[RO_A3S], T3u = tot[RO_A3U],
                T4s = tot[RO_A4S];

  // ---- the passes, a chunk of W targets at a time
  int carry[RO_NA] = {0, 0, 0, 0, 0, 0}, carry5s = 0, carry5u = 0;
  int32_t planned = 0;
  for (int c = 0; __any(c < ns); c += W) {
    const int i = c + gl;
    const bool live = i < ns;
    if (live && ns > W) t = ro_load(d, lo + i);  // (an object of one chunk still holds its targets)
#pragma unroll
    for (int k = 0; k < RO_NA; ++k) a[k] = 0;
    if (live) ro_offers(t, a);
    int x[RO_NA];
#pragma unroll
    for (int k = 0; k < RO_NA; ++k) x[k] = ro_prefix<W>(a[k], gl, carry[k]);
    RoPlan p{0, 0, 0, 0};
    int32_t sm, um, lu5 = 0, a5s = 0, a5u = 0;
    const bool work = live && !scaling;
    if (work) {
      if (t.cls == RO_CLS_OUT) {
        const int32_t S1 = ro_budget(S0, x[RO_A1S]), U1 = ro_budget(U0, x[RO_A1U]);
        if (!ro_skip_update(t, S1, U1)) {
          p = RoPlan{t.r, 0, 0, RO_HAS_REPLICAS};
          ro_fenceposts(t, S1, U1, t.lu, p_surge, p, sm, um);
        }
        const int32_t S4 = ro_budget(S0, T1s + T3s + x[RO_A4S]);
        if (!(S4 <= 0 && t.ls <= 0) && (t.upd || t.r == 0)) {
          p.r = ro_add(t.r, ro_scale_out(S4, t.during ? 0 : t.ls, t).res);
          p.f |= RO_PLANNED | RO_HAS_REPLICAS;
        }
      } else if (t.cls == RO_CLS_UPDATE) {
        const int32_t S3 = ro_budget(S0, T1s + x[RO_A3S]), U3 = ro_budget(U0, T1u + T2u + x[RO_A3U]);
        if (!ro_skip_update(t, S3, U3)) ro_fenceposts(t, S3, U3, t.lu, p_surge, p, sm, um);
      } else {
        const int32_t U2 = ro_budget(U0, T1u + x[RO_A2U]);
        if (!(U2 <= 0 && t.lu <= 0))
          p = RoPlan{ro_sub(t.r, ro_scale_in(U2, t.during ? 0 : t.lu, t).res), 0, 0,
                     RO_PLANNED | RO_HAS_REPLICAS | RO_ONLY_PATCH_REPLICAS};
        lu5 = ro_lu5(t, (p.f & RO_PLANNED) ? p.r : t.r);
        a5s = ro_offer(t.rtu, t.ls);
        a5u = ro_offer(t.rtua, lu5);
      }
    }
    const int x5s = ro_prefix<W>(a5s, gl, carry5s), x5u = ro_prefix<W>(a5u, gl, carry5u);
    if (work && t.cls == RO_CLS_IN) {
      const int32_t S5 = ro_budget(S0, T1s + T3s + T4s + x5s), U5 = ro_budget(U0, T1u + T2u + T3u + x5u);
      if (!ro_skip5(t, S5, U5, lu5)) {
        if (!(p.f & RO_PLANNED)) p = RoPlan{t.r, 0, 0, RO_HAS_REPLICAS};
        p.f &= (uint8_t)~RO_ONLY_PATCH_REPLICAS;
        ro_fenceposts(t, S5, U5, lu5, p_surge, p, sm, um);
      }
    }
    if (live) {
      if (scaling) p.f = RO_PLANNED;
      ro_store(d, lo + i, t.f, p);
      planned = ro_add(planned, ro_planned_replicas(t, p));
    }
  }
  if (W > 1) planned = ro_group_sum<W>(planned);
  if (o >= 0 && !err && !serial) {
    const bool invalid = !scaling && ro_invalid(p_rep, p_ms, p_mu, planned, desired, sum_r);
    if (invalid) ro_store_unplanned(d, lo, lo + n, gl, W);  // validatePlans failed: RolloutPlans{}
    if (gl == 0) d.status[o] = scaling ? RO_SCALE : invalid ? RO_INVALID : RO_OK;
  }
}

template <int W>
__global__ __launch_bounds__(256) void rollout_kernel(RolloutDev d, int long_grid) {
  if ((int)blockIdx.x < long_grid) {
    // ---- long path: one listed object per wave
    const int w = (int)blockIdx.x * 4 + ((int)threadIdx.x >> 6);
    plan_group<64>(d, w < d.n_long ? d.long_list[w] : -1, (int)threadIdx.x & 63);
    return;
  }
  // ---- group path: the loop is uniform over the wave (groups past O idle)
  constexpr int GPB = 256 / W;
  const int gl = (int)threadIdx.x & (W - 1), g = (int)threadIdx.x / W;
  const int64_t stride = (int64_t)((int)gridDim.x - long_grid) * GPB;
  for (int64_t base = (int64_t)((int)blockIdx.x - long_grid) * GPB; base < d.O; base += stride) {
    const int64_t o64 = base + g;
    int o = o64 < d.O ? (int)o64 : -1;
    if (o >= 0 && (d.obj_mode[o] & RO_MODE_LONG)) o = -1;
    plan_group<W>(d, o, gl);
  }
}

hipError_t launch_rollout(const RolloutDev& d, const RolloutRoute& r, hipStream_t st) {
  (void)hipGetLastError();
  const unsigned grid = (unsigned)(r.grid + r.long_grid);
  if (grid > 0)
    with_width<1>(r.width, [&](auto W) {
      hipLaunchKernelGGL((rollout_kernel<decltype(W)::value>), dim3(grid), dim3(256), 0, st, d, r.long_grid);
    });
  return hipGetLastError();
}

}  // namespace kad

// ------------------------------------------------------ host half: kad_rollout_*
#include "kad_arena.h"

using namespace kad;

namespace {

// what the validation leaves for the launch: each object's path, the objects of the long path, the counts
struct RolloutPlanHost {
  std::vector<uint8_t> obj_mode;
  std::vector<int32_t> long_list;
  int64_t short_targets = 0;
  int n_serial = 0;
};

int64_t abs64(int32_t v) { return v < 0 ? -(int64_t)v : (int64_t)v; }

}  // namespace

extern "C" {

// The counts, the offset array monotone from 0 and ending at n_targets, every flag known and consistent (a target
// without a member object has an all-zero status and is not to delete; a target to delete desires 0), the outputs:
// all of it on the host, before anything is copied or launched. With a plan the same pass leaves each object's
// path: long (more than long_min targets), serial (the absolute values of its inputs sum to RO_NOWRAP_BELOW or
// more, or force_serial). nowrap[O], where given, is 1 for the objects that may take the prefix-sum form.
static int validate_rollout(const kad_rollout_batch* b, const kad_rollout_view* out, int long_min, bool force_serial,
                            RolloutPlanHost* plan, uint8_t* nowrap, std::string* err) {
  auto bad = [&](const char* m) {
    *err = m;
    return KAD_EINVAL;
  };
  const int64_t O = b->n_objects, T = b->n_targets;
  if (O < 0 || T < 0) return bad("negative count");
  if (!b->obj_tgt_off) return bad("offset array missing");
  if (O && (!b->obj_max_surge || !b->obj_max_unavailable || !b->obj_replicas || !b->obj_flags)) return bad("input array missing");
  if (T && (!b->tgt_vals || !b->tgt_flags)) return bad("input array missing");
  const int32_t* to = b->obj_tgt_off;
  if (off_bad(to, O)) return bad("obj_tgt_off not monotone from 0");
  if (to[O] != T) return bad("obj_tgt_off does not end at n_targets");
  const uint8_t *of = b->obj_flags, *tf = b->tgt_flags;
  const int32_t* tv = b->tgt_vals;
  if (first_bad(O, [&](int64_t i) { return (of[i] & ~KAD_ROLLOUT_OBJ_ERROR) != 0; }) >= 0) return bad("obj_flags: unknown flag");
  constexpr uint8_t TGT_ALL = KAD_ROLLOUT_TGT_UPDATED | KAD_ROLLOUT_TGT_EXISTS | KAD_ROLLOUT_TGT_TO_DELETE;
  if (first_bad(T, [&](int64_t i) { return (tf[i] & ~TGT_ALL) != 0; }) >= 0) return bad("tgt_flags: unknown flag");
  if (first_bad(T, [&](int64_t i) {
        if (tf[i] & KAD_ROLLOUT_TGT_EXISTS) return false;
        if (tf[i]) return true;
        for (int v = 0; v < RO_DESIRED; ++v)
          if (tv[(int64_t)v * T + i]) return true;
        return false;
      }) >= 0)
    return bad("a target without a member object is UPDATED, TO_DELETE or has a status");
  if (first_bad(T, [&](int64_t i) { return (tf[i] & KAD_ROLLOUT_TGT_TO_DELETE) && tv[(int64_t)RO_DESIRED * T + i] != 0; }) >= 0)
    return bad("a target to delete desires replicas");
  if (!out || (O && !out->status) ||
      (T && (!out->replicas || !out->max_surge || !out->max_unavailable || !out->plan_flags || !out->action)))
    return bad("output view missing");
  if (plan) plan->obj_mode.assign((size_t)O, 0);
  for (int64_t i = 0; i < O; ++i) {
    const bool error = (of[i] & KAD_ROLLOUT_OBJ_ERROR) != 0;
    int64_t sum = abs64(b->obj_max_surge[i]) + abs64(b->obj_max_unavailable[i]) + abs64(b->obj_replicas[i]);
    for (int v = 0; v < RO_NV && sum < RO_NOWRAP_BELOW; ++v)
      for (int64_t k = to[i]; k < to[i + 1] && sum < RO_NOWRAP_BELOW; ++k) sum += abs64(tv[(int64_t)v * T + k]);
    const bool nw = sum < RO_NOWRAP_BELOW;
    if (nowrap) nowrap[i] = nw ? 1 : 0;
    if (!plan || error) continue;  // an object in error is passed through on the group path, whatever its length
    const int64_t n = to[i + 1] - to[i];
    uint8_t m = 0;
    if (!nw || force_serial) {
      m |= RO_MODE_SERIAL;
      ++plan->n_serial;
    }
    if (n > long_min) {
      m |= RO_MODE_LONG;
      plan->long_list.push_back((int32_t)i);
    } else {
      plan->short_targets += n;
    }
    plan->obj_mode[(size_t)i] = m;
  }
  return KAD_OK;
}

static int rollout_plan_locked(kad_ctx* c, const kad_rollout_batch* b, const kad_rollout_view* out) {
  Stage& stg = c->stage[STG_ROLLOUT];
  const int long_min = stg.force.long_min_or(RO_LONG_MIN);
  std::string err;
  RolloutPlanHost plan;
  if (int r = validate_rollout(b, out, long_min, stg.force.serial != 0, &plan, nullptr, &err)) return fail(c, r, err);
  const int O = b->n_objects, T = b->n_targets;
  if (O == 0) return KAD_OK;
  HIPCHK(c, hipSetDevice(c->device));
  const int n_long = (int)plan.long_list.size();
  RolloutRoute route = route_rollout(O, n_long, plan.short_targets, plan.n_serial, n_cus());
  group_force_apply(stg.force, n_long < O, O, n_cus(), route.width, route.grid, &route.stride);
  route.long_min = long_min;
  // one buffer: the inputs, then the outputs
  const size_t o = (size_t)O, t = (size_t)T, nl = (size_t)n_long;
  RolloutDev d{};
  d.O = O;
  d.T = T;
  d.n_long = n_long;
  Arena a;
  a.in(d.obj_tgt_off, b->obj_tgt_off, o + 1);
  a.in(d.obj_max_surge, b->obj_max_surge, o);
  a.in(d.obj_max_unavailable, b->obj_max_unavailable, o);
  a.in(d.obj_replicas, b->obj_replicas, o);
  a.in(d.obj_flags, b->obj_flags, o);
  a.in(d.tgt_vals, b->tgt_vals, (size_t)RO_NV * t);
  a.in(d.tgt_flags, b->tgt_flags, t);
  a.in(d.obj_mode, plan.obj_mode.data(), o);
  a.in(d.long_list, plan.long_list.data(), nl);
  a.out(d.replicas, out->replicas, t);
  a.out(d.max_surge, out->max_surge, t);
  a.out(d.max_unavailable, out->max_unavailable, t);
  a.out(d.plan_flags, out->plan_flags, t);
  a.out(d.action, out->action, t);
  a.out(d.status, out->status, o);
  if (int r = a.commit(c, stg.buf)) return r;
  HIPCHK(c, hipEventRecord(stg.ev[0], c->stream));
  HIPCHK(c, launch_rollout(d, route, c->stream));
  HIPCHK(c, hipEventRecord(stg.ev[1], c->stream));
  stage_ran(stg, route);
  if (int r = a.fetch(c)) return r;
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return KAD_OK;
}

int kad_rollout_check(const kad_rollout_batch* b, const kad_rollout_view* out, uint8_t* nowrap) {
  return check_guarded([&]() -> int {
    if (!b) return KAD_EINVAL;
    std::string err;
    return validate_rollout(b, out, RO_LONG_MIN, false, nullptr, nowrap, &err);
  });
}

int kad_rollout_plan(kad_ctx* c, const kad_rollout_batch* b, const kad_rollout_view* out) {
  return entry(c, b != nullptr, [&]() -> int {
    return rollout_plan_locked(c, b, out);
  });
}

int kad_rollout_timing(kad_ctx* c, float ms[1]) { return stage_timing(c, STG_ROLLOUT, 1, ms, "no kad_rollout_plan ran"); }

int kad_rollout_route_eval(int32_t n_objects, int32_t n_long, int64_t short_targets, int32_t n_serial, int32_t n_cu, int32_t* out) {
  if (!out || n_objects < 0 || n_long < 0 || n_long > n_objects || short_targets < 0 || n_serial < 0 || n_serial > n_objects ||
      n_cu < 1)
    return KAD_EINVAL;
  return route_record<KAD_ROLLOUT_ROUTE_FIELDS>(out, route_rollout(n_objects, n_long, short_targets, n_serial, n_cu));
}

int kad_rollout_last_route(kad_ctx* c, int32_t* out) { return stage_last_route(c, STG_ROLLOUT, out, "no kad_rollout_plan ran"); }

int kad_rollout_debug_route(kad_ctx* c, int32_t force_width, int32_t force_long_min, int32_t force_serial) {
  return stage_debug_route(c, STG_ROLLOUT, group_width_ok(force_width, 1) && (force_serial == 0 || force_serial == 1),
                           GroupForce{force_width, force_long_min, force_serial});
}

}  // extern "C"
