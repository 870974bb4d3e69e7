// Stand-alone stage entry points: select_rows_kernel, plan_rows_kernel.
// Part of kad_kernels.hip's translation unit, which includes the kernels' headers in definition order.
#pragma once

#include "kad_device.h"
#include "kad_k_plan.h"
#include "kad_plan.h"
#include "kad_select.h"
#include "kad_wave.h"

namespace kad {

template <bool GSCR>
__global__ __launch_bounds__(64) void select_rows_kernel(int n_rows, const int32_t* row_off, const int64_t* scores,
                                                         const int64_t* maxc, uint32_t pflags, int32_t* out_count,
                                                         int32_t* out_sel, int32_t* out_status, char* gscratch,
                                                         int wave_bytes, int kmax, int r_stride) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int lane = lane_id();
  char* region = GSCR ? gscratch + (size_t)blockIdx.x * wave_bytes : smem;
  const RowLayout L = row_layout(kmax);
  int64_t* tot = (int64_t*)(region + L.tot);
  uint16_t* perm = (uint16_t*)(region + L.perm);
  uint64_t* selb = (uint64_t*)(region + L.sel);
  uint32_t* hist = (uint32_t*)(region + L.hist);
  uint16_t* posl = (uint16_t*)(region + L.posl);
  uint16_t* posr = (uint16_t*)(region + L.posr);
  const int xs_b = (pflags & KAD_PROFILE_XORSHIFT_GO121) ? 7 : 17;
  const int xs_c = (pflags & KAD_PROFILE_XORSHIFT_GO121) ? 17 : 5;
  for (int r = blockIdx.x; r < n_rows; r += r_stride) {
    const int a = row_off[r], n = row_off[r + 1] - a;
    const int64_t mc = maxc[r];
    if (mc < 0) {
      if (lane == 0) {
        out_status[r] = KAD_ST_ERR_SELECT;
        out_count[r] = 0;
      }
      continue;
    }
    int64_t rmin = I64_MAX, rmax = I64_MIN;
    for (int j = lane; j < n; j += WAVE) {
      const int64_t t = scores[a + j];
      tot[j] = t;
      rmin = t < rmin ? t : rmin;
      rmax = t > rmax ? t : rmax;
    }
    rmin = wave_min_i64(rmin);
    rmax = wave_max_i64(rmax);
    wsync<GSCR>();
    const int64_t k = mc < n ? mc : n;
    SelWs ws{tot, selb, perm, hist, posl, posr};
    select_topk<GSCR>(ws, n, k, rmin, rmax, xs_b, xs_c);
    int base = 0;
    for (int jc = 0; jc < ((n + 63) >> 6); ++jc) {
      const uint64_t m = selb[jc];
      if ((m >> lane) & 1) out_sel[a + base + mbcnt(m)] = jc * WAVE + lane;
      base += popc64(m);
    }
    if (lane == 0) {
      out_status[r] = KAD_ST_OK;
      out_count[r] = base;
    }
    wsync<GSCR>();
  }
}

template <bool GSCR>
__global__ __launch_bounds__(64) void plan_rows_kernel(PlanRowsDev R, char* gscratch, int wave_bytes, int r_stride,
                                                       int force_ws) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int lane = lane_id();
  char* region = GSCR ? gscratch + (size_t)blockIdx.x * wave_bytes : smem;
  // one row with the whole wave: the register planner for K <= 64 (plan_kernel's path), else (or with
  // force_ws == 1) the LDS-workspace planner
  auto one_row = [&](int r) {
    const int a = R.row_off[r], K = R.row_off[r + 1] - a;
    if (K <= 0) return;
    if (K <= WAVE && force_ws != 1) {
      const bool v = lane < K;
      PlanLane e{0, 0, 0, 0, 0, 0u, 0u};
      if (v) {
        e.hash = R.hash[a + lane];
        e.w = R.weight[a + lane];
        e.mn = R.min_r[a + lane];
        e.mx = R.max_r[a + lane];
        e.cap = R.cap[a + lane];
        e.cur = R.current[a + lane];
        e.fl = R.elem_flags[a + lane] & (EF_HAS_MAX | EF_HAS_CAP);
      }
      PlanOut po;
      plan_row_lanes(e, K, R.total[r], R.row_flags[r] & 1, (R.row_flags[r] >> 1) & 1, po);
      if (v) {
        R.out_plan[a + lane] = po.plan;
        R.out_overflow[a + lane] = (po.ofl & EF_HAS_OVER) ? po.over : -1;
      }
      return;
    }
    PlanWs ws = plan_ws(region, K);
    for (int i = lane; i < K; i += WAVE) {
      ws.cid[i] = i;
      ws.hash[i] = R.hash[a + i];
      ws.w[i] = R.weight[a + i];
      ws.mn[i] = R.min_r[a + i];
      ws.mx[i] = R.max_r[a + i];
      ws.cap[i] = R.cap[a + i];
      ws.cur[i] = R.current[a + i];
      ws.fl[i] = R.elem_flags[a + i] & (EF_HAS_MAX | EF_HAS_CAP);
    }
    wsync<GSCR>();
    plan_row<GSCR>(ws, K, R.total[r], R.row_flags[r] & 1, (R.row_flags[r] >> 1) & 1);
    for (int i = lane; i < K; i += WAVE) {
      R.out_plan[a + i] = ws.plan[i];
      R.out_overflow[a + i] = (ws.ofl[i] & EF_HAS_OVER) ? ws.over[i] : -1;
    }
    wsync<GSCR>();
  };
  if (force_ws == 2 && !GSCR) {  // rows r, r + 1 together in the two half-waves when both hold <= 32 elements (plan_row_pair)
    uint64_t* kbuf = (uint64_t*)region;
    const int sl = lane & 31;
    for (int r = 2 * (int)blockIdx.x; r < R.n_rows; r += 2 * r_stride) {
      const int KA = R.row_off[r + 1] - R.row_off[r];
      const int KB = r + 1 < R.n_rows ? R.row_off[r + 2] - R.row_off[r + 1] : 0;
      if (KA > 32 || KB > 32) {
        one_row(r);
        if (r + 1 < R.n_rows) one_row(r + 1);
        continue;
      }
      const int rr = lane >= 32 ? r + 1 : r;
      const int K = lane >= 32 ? KB : KA;
      const int a = rr < R.n_rows ? R.row_off[rr] : 0;
      const bool v = sl < K;
      PlanLane e{0, 0, 0, 0, 0, 0u, 0u};
      if (v) {
        e.hash = R.hash[a + sl];
        e.w = R.weight[a + sl];
        e.mn = R.min_r[a + sl];
        e.mx = R.max_r[a + sl];
        e.cap = R.cap[a + sl];
        e.cur = R.current[a + sl];
        e.fl = R.elem_flags[a + sl] & (EF_HAS_MAX | EF_HAS_CAP);
      }
      const uint32_t rf = K > 0 ? R.row_flags[rr] : 0u;
      PlanOut po;
      plan_row_pair(e, K, K > 0 ? R.total[rr] : 0, rf & 1, (rf >> 1) & 1, po, kbuf);
      if (v) {
        R.out_plan[a + sl] = po.plan;
        R.out_overflow[a + sl] = (po.ofl & EF_HAS_OVER) ? po.over : -1;
      }
    }
    return;
  }
  for (int r = blockIdx.x; r < R.n_rows; r += r_stride) one_row(r);
}

}  // namespace kad
