// kad_rollout_plan (kad_rollout.hip): one batch of federated Deployments and their (object, member cluster)
// targets, the arithmetic of RolloutPlanner.Plan shared by the device and the host, the launch decision, the launch.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kad_groups.h"

namespace kad {

// rows of tgt_vals: TargetStatus (pkg/controllers/util/rolloutplan.go:166-177) without Updated, then DesiredReplicas
enum RoCol { RO_REPLICAS, RO_ACTUAL, RO_AVAILABLE, RO_UPDATED, RO_UPDATED_AVAILABLE, RO_CURRENT_NEW,
             RO_CURRENT_NEW_AVAILABLE, RO_MAX_SURGE, RO_MAX_UNAVAILABLE, RO_DESIRED, RO_NV };
constexpr uint8_t RO_OBJ_ERROR = 1;                                          // KAD_ROLLOUT_OBJ_*
constexpr uint8_t RO_TGT_UPDATED = 1, RO_TGT_EXISTS = 2, RO_TGT_TO_DELETE = 4;  // KAD_ROLLOUT_TGT_*
constexpr uint8_t RO_PLANNED = 1, RO_HAS_REPLICAS = 2, RO_HAS_SURGE = 4, RO_HAS_UNAVAILABLE = 8,
                  RO_ONLY_PATCH_REPLICAS = 16;                               // KAD_ROLLOUT_PLAN_*
enum RoAction { RO_KEEP_TEMPLATE_PATCH, RO_NONE, RO_DELETE, RO_CREATE, RO_PATCH_REPLICAS, RO_UPDATE };  // KAD_ROLLOUT_ACT_*
enum RoStatus { RO_OK, RO_SCALE, RO_INVALID, RO_ERROR };                                              // KAD_ROLLOUT_ST_*
constexpr uint8_t RO_MODE_LONG = 1, RO_MODE_SERIAL = 2;  // RolloutDev::obj_mode
constexpr int RO_LONG_MIN = 256;  // objects with more targets than this go one per wave (a starting value)
// An object whose inputs' absolute values sum to less than this cannot wrap int32 anywhere in Plan(): a budget is
// bounded by twice that sum, a budget plus a target's least surge by three times, a budget less everything every
// pass may take by four times. Only such objects take the prefix-sum form.
constexpr int64_t RO_NOWRAP_BELOW = (int64_t)1 << 29;

struct RolloutDev {
  int O, T;
  int n_long;
  const int32_t* obj_tgt_off;   // [O + 1]
  const int32_t* obj_max_surge, *obj_max_unavailable, *obj_replicas;  // [O]
  const uint8_t* obj_flags;     // [O]
  const int32_t* tgt_vals;      // [RO_NV][T]
  const uint8_t* tgt_flags;     // [T]
  // built on the host while it validates
  const uint8_t* obj_mode;      // [O] RO_MODE_*
  const int32_t* long_list;     // [n_long] the objects of the long path, ascending
  int32_t *replicas, *max_surge, *max_unavailable;  // [T]
  uint8_t *plan_flags, *action;  // [T]
  uint8_t* status;              // [O]
};

// ---------------------------------------------------------------- Go int32 arithmetic (wraps; never signed overflow)
#define KAD_HD __host__ __device__ __forceinline__
KAD_HD int32_t ro_add(int32_t a, int32_t b) { return (int32_t)((uint32_t)a + (uint32_t)b); }
KAD_HD int32_t ro_sub(int32_t a, int32_t b) { return (int32_t)((uint32_t)a - (uint32_t)b); }
KAD_HD int32_t ro_min(int32_t a, int32_t b) { return b < a ? b : a; }
KAD_HD int32_t ro_max(int32_t a, int32_t b) { return b > a ? b : a; }
KAD_HD int32_t ro_pos(int32_t a) { return a < 0 ? 0 : a; }

// one target's inputs and every term of TargetInfo's helpers (rolloutplan.go:255-332) that depends on them alone
struct RoTarget {
  int32_t r, act, av, ur, uar, cn, cna, ms, mu, d;
  uint8_t f;
  int32_t rtu, rtua;  // ReplicasToUpdate, ReplicasToUpdatedAvailable
  int32_t ls, lu;     // LeastSurge, LeastUnavailable
  bool upd, during, completed, is_surge;
  int cls;            // sortTargets: 0 to update, 1 to scale out, 2 to scale in
};
enum { RO_CLS_UPDATE, RO_CLS_OUT, RO_CLS_IN };

KAD_HD void ro_derive(RoTarget& t) {
  t.upd = (t.f & RO_TGT_UPDATED) != 0;
  t.rtu = ro_pos(ro_sub(t.r, t.ur));
  t.rtua = ro_pos(ro_sub(t.r, t.uar));
  const int32_t rtuc = ro_pos(ro_sub(t.r, t.cn)), rtuac = ro_pos(ro_sub(t.r, t.cna));
  t.during = t.cn < t.r || (t.upd && t.rtu > 0);
  t.ls = ro_pos(ro_sub(t.act, t.r));
  t.lu = ro_pos(ro_sub(t.r, t.av));
  if (t.during) {
    t.ls = ro_max(t.ls, ro_min(t.ms, ro_add(t.ls, rtuc)));
    t.lu = ro_max(t.lu, ro_min(t.mu, rtuac));
  }
  t.completed = t.rtu == 0;
  t.is_surge = t.ms != 0 && t.mu == 0;
  const int32_t change = ro_sub(t.d, t.r);
  t.cls = change < 0 ? RO_CLS_IN : change > 0 ? RO_CLS_OUT : RO_CLS_UPDATE;
}
KAD_HD bool ro_flip(const RoTarget& t, bool p_surge) { return t.is_surge && !p_surge && t.rtua > 0; }

struct RoFence {
  int32_t res, more;
};
// TargetInfo.MaxSurge / MaxUnavailable (:193-225): `to` is ReplicasToUpdate / ReplicasToUpdatedAvailable, `cur` the
// member's own maxSurge / maxUnavailable
KAD_HD RoFence ro_fence(int32_t m, int32_t least, int32_t to, int32_t cur) {
  int32_t res = ro_pos(ro_min(ro_add(m, least), to));
  const int32_t more = ro_pos(ro_sub(res, least));
  if (m < 0 && least > cur && res > cur) res = cur;
  return RoFence{res, more};
}
KAD_HD RoFence ro_scale_out(int32_t m, int32_t least, const RoTarget& t) {  // MaxScaleOut (:227-237)
  const int32_t res = ro_pos(ro_min(ro_add(m, least), ro_sub(t.d, t.r)));
  return RoFence{res, ro_pos(ro_sub(res, least))};
}
KAD_HD RoFence ro_scale_in(int32_t m, int32_t least, const RoTarget& t) {  // MaxScaleIn (:239-253)
  int32_t res = ro_min(ro_add(m, least), ro_sub(t.r, t.d));
  if (res > t.r) res = t.r;
  res = ro_pos(res);
  return RoFence{res, ro_pos(ro_sub(res, least))};
}

// a target's plan while the passes build it
struct RoPlan {
  int32_t r, s, u;
  uint8_t f;  // RO_PLANNED ...
};
// the surge / unavailable half of passes 1, 3 and 5 (:591-599, :628-635, :681-687): both fenceposts from the two
// budgets, then correctFencepost (:93-112). Returns what the budgets lose.
KAD_HD void ro_fenceposts(const RoTarget& t, int32_t S, int32_t U, int32_t lu, bool p_surge, RoPlan& p, int32_t& sm, int32_t& um) {
  const RoFence s = ro_fence(S, t.ls, t.rtu, t.ms), u = ro_fence(U, lu, t.rtua, t.mu);
  sm = s.more;
  um = u.more;
  p.s = s.res;
  p.u = u.res;
  p.f |= RO_PLANNED | RO_HAS_SURGE | RO_HAS_UNAVAILABLE;
  if (t.completed && !ro_flip(t, p_surge)) {
    p.f &= (uint8_t)~(RO_HAS_SURGE | RO_HAS_UNAVAILABLE);
    p.s = p.u = 0;
  } else if (p.s == 0 && p.u == 0) {
    if (t.is_surge)
      p.s = 1;
    else
      p.u = 1;
  }
}
KAD_HD bool ro_skip_update(const RoTarget& t, int32_t S, int32_t U) {  // SkipPlanForUpdate (:334-337)
  return S <= 0 && U <= 0 && !t.upd && !t.during && t.ls <= 0 && t.lu <= 0;
}
// pass 5's leastUnavailable (:669-675): what pass 2 scaled in is excluded
KAD_HD int32_t ro_lu5(const RoTarget& t, int32_t plan_r) {
  int32_t lu = t.lu;
  if (!t.during) lu = ro_pos(ro_sub(lu, ro_sub(t.r, plan_r)));
  return lu;
}
KAD_HD bool ro_skip5(const RoTarget& t, int32_t S, int32_t U, int32_t lu5) {  // SkipPlanForUpdateForThoseToScaleIn (:339-354)
  if (S <= 0 && U <= 0 && !t.upd && !t.during) {
    if (lu5 > 0) return false;
    const int32_t ls = t.d < t.r ? 0 : t.ls;
    return !(ls > 0);
  }
  return false;
}
// the replicas validatePlans counts for a target (:836-853)
KAD_HD int32_t ro_planned_replicas(const RoTarget& t, const RoPlan& p) {
  if (!(p.f & RO_PLANNED)) return t.r;
  return (p.f & RO_HAS_REPLICAS) ? p.r : t.d;
}
KAD_HD bool ro_invalid(int32_t p_rep, int32_t p_ms, int32_t p_mu, int32_t planned, int32_t desired, int32_t current) {  // :855-866
  if (ro_sub(p_rep, desired) > p_mu) return true;
  const int32_t l = desired > current ? current : desired, h = desired > current ? desired : current;
  return ro_sub(l, planned) > p_mu || ro_sub(planned, h) > p_ms;
}
// the dispatch operation that follows (pkg/controllers/sync/dispatch/managed.go:219-249)
KAD_HD uint8_t ro_action(uint8_t tf, const RoPlan& p) {
  if (!(p.f & RO_PLANNED)) return (tf & RO_TGT_EXISTS) ? RO_KEEP_TEMPLATE_PATCH : RO_NONE;
  const bool has_r = (p.f & RO_HAS_REPLICAS) != 0;
  if ((tf & RO_TGT_TO_DELETE) && (!has_r || p.r == 0)) return RO_DELETE;
  if (!(tf & RO_TGT_EXISTS)) return RO_CREATE;
  if ((p.f & RO_ONLY_PATCH_REPLICAS) && has_r) return RO_PATCH_REPLICAS;
  return RO_UPDATE;
}
// a budget after `used` was offered to it by the targets before (each takes min(budget, its offer) while the budget
// is positive and nothing otherwise): only where nothing wraps
KAD_HD int32_t ro_budget(int32_t m0, int64_t used) {
  if (m0 <= 0) return m0;
  const int64_t m = (int64_t)m0 - used;
  return m > 0 ? (int32_t)m : 0;
}
// what a target offers to take from the budgets in each pass (0 outside the pass's class)
KAD_HD int32_t ro_offer(int32_t to, int32_t least) { return ro_pos(ro_sub(to, least)); }

// The launch decision of one kad_rollout_plan, taken here and nowhere else (kad_rollout_route_eval /
// kad_rollout_last_route show it). Group path: a wave is 64 / width lane groups, every group takes one object at a
// time, a target per lane, objects with more targets than the width in chunks of it; the groups of a grid stride
// over the objects. The width is the mean targets per short object rounded up to a power of two in [1, 64].
// Objects with more than long_min targets (the caller counts them: n_long, and the short objects' targets) are
// left out there and go one per wave, four waves a block. n_serial objects walk serially on one lane.
struct RolloutRoute {
  int32_t width;      // lanes per object on the group path
  int32_t long_min;   // an object with more targets than this is on the long path
  int32_t threads;    // per block
  int32_t grid;       // blocks of the group path (0 when every object is long)
  int32_t long_grid;  // blocks of the long path = ceil(n_long / 4)
  int32_t stride;     // objects between two consecutive objects of one lane group
  int32_t serial;     // objects on the serial walk
};

inline RolloutRoute route_rollout(int O, int n_long, int64_t short_targets, int n_serial, int n_cu) {
  RolloutRoute r{};
  const int n_short = O - n_long;
  r.width = group_width(short_targets, n_short, 1, 1);
  r.long_min = RO_LONG_MIN;
  r.threads = 256;
  r.grid = n_short > 0 ? group_grid(O, r.width, n_cu) : 0;  // no LDS
  r.long_grid = (n_long + 3) / 4;
  r.stride = group_stride(r.grid, r.width);
  r.serial = n_serial;
  return r;
}

hipError_t launch_rollout(const RolloutDev& d, const RolloutRoute& r, hipStream_t st);

}  // namespace kad
