// The monitor controller (kad_monitor_*): one meter per federated object in a device-resident table, a batch of
// object events against it, and the report's pass over it.
//
// MonitorSubController.reconcile (pkg/controllers/monitor/monitor_subcontroller.go:172-343) updates one BaseMeter per
// event; DoReport (report.go:31-163) walks every meter each ReportInterval. Both restated line by line, with `now` an
// argument and time as kad_monitor.h declares it:
//
//   monitor_reconcile_kernel<W>  blocks below n_long: one listed long object per 256-thread block; the other blocks: a
//                        wave is 64 / W lane groups, each group takes one object at a time. The two reflect.DeepEqual
//                        (:319, :326) are "same length and equal entry by entry": the lanes stride over both lists
//                        and a ballot says whether any differed. The group's lane 0 runs the state machine and writes
//                        the slot's columns in place. Slots are distinct within a call, so no two groups share one.
//   monitor_scan_kernel<PATH>    the report's one pass: a lane reads MON_VEC consecutive slots of every column (16 B a
//                        load), the blocks stride over the table. The 12 bucket counts and the 2 throughputs are
//                        ballots and popcounts per wave, summed in LDS per block, one atomic per block and counter;
//                        the per-type five-minute counts go to block-private LDS bins (n_types <= MON_LDS_TYPES) or
//                        to global atomics; every wave tile (256 slots) leaves its number of timers.
//   monitor_offsets_kernel       one wave: the exclusive sums of the tiles' timer counts, and the totals.
//   monitor_scatter_kernel       the tiles that have timers are read again and their (slot, ms) entries written at
//                        their tile's offset plus their rank within the tile: ascending slot order.
//   monitor_io_kernel<LOAD>      kad_monitor_load / kad_monitor_read: a lane per listed slot.
//
// Integers only; every atomic is a relaxed add whose result nobody reads before its kernel ends, so nothing depends
// on an order of arrival. Ordinary vector stores. Nothing here touches state that kad_schedule reads.
#include "kad_monitor.h"
#include "kad_wave.h"

namespace kad {

namespace {

__device__ __forceinline__ bool mon_near(int64_t t) { return t < MON_NEAR; }
// Go's Time.Sub: the plain difference, saturated when the operands are too far apart for a Duration
__device__ __forceinline__ int64_t mon_sub(int64_t a, int64_t b) {
  const bool az = mon_near(a), bz = mon_near(b);
  if (az != bz) return az ? I64_MIN : I64_MAX;
  return a - b;
}

// does any lane of this lane's group of W hold p (W == 256: of the block)
template <int W>
__device__ __forceinline__ bool grp_any(bool p) {
  if constexpr (W == 256) {
    return __syncthreads_or(p ? 1 : 0) != 0;
  } else {
    const uint64_t m = ballot(p);
    if constexpr (W == 64) return m != 0;
    return ((m >> (lane_id_h() & ~(W - 1) & 63)) & ((1ull << (W & 63)) - 1)) != 0;
  }
}

// reflect.DeepEqual of two maps held as lists that ascend by cluster id: every lane of the group calls it
template <int W>
__device__ __forceinline__ bool lists_equal(const MonList& a, const MonList& b, int o, int gl) {
  const int a_lo = a.off[o], n = a.off[o + 1] - a_lo, b_lo = b.off[o];
  if (n != b.off[o + 1] - b_lo) return false;
  bool diff = false;
  for (int i = gl; i < n; i += W)
    diff |= a.cluster[a_lo + i] != b.cluster[b_lo + i] || a.gen[a_lo + i] != b.gen[b_lo + i];
  return !grp_any<W>(diff);
}

// One object, by its W lanes.
template <int W>
__device__ __forceinline__ void mon_object(const MonRecDev& d, const int o, const int gl) {
  const bool eq_cf = lists_equal<W>(d.mem, d.fed, o, gl);   // DeepEqual(clusterStatus, fedStatus), :319
  const bool eq_lc = lists_equal<W>(d.last, d.mem, o, gl);  // DeepEqual(lastStatus, clusterStatus), :326
  if (gl != 0) return;
  const uint16_t f = d.obj_flags[o];
  const int64_t slot = d.slot[o], now = d.now;
  int64_t* const meter = d.meter + (int64_t)o * MON_COLS;
  int64_t* const would = d.would + (int64_t)o * 2;
  if (f & MON_DELETED) {  // :182-191
    d.t.flags[slot] = 0;
    d.result[o] = MON_ALL_OK;
    d.bits[o] = MON_METER_DELETED;
#pragma unroll
    for (int k = 0; k < MON_COLS; ++k) meter[k] = 0;
    would[0] = would[1] = 0;
    return;
  }
  int64_t cr, lu, ss, lst, oos;
  if (f & MON_NEW) {  // :193-195
    cr = d.creation[o];
    lu = ss = lst = MON_ZERO;
    oos = 0;
  } else {
    cr = d.t.col[MON_CR][slot];
    lu = d.t.col[MON_LU][slot];
    ss = d.t.col[MON_SS][slot];
    lst = d.t.col[MON_LST][slot];
    oos = d.t.col[MON_OOS][slot];
  }
  // ---- reconcileSync, :255-300
  if (f & MON_SS_PARSED) ss = d.sync_success[o];
  bool update = true;
  const bool lssg = (f & MON_LSSG_PRESENT) && (f & MON_LSSG_EQUAL);
  if (f & MON_LASTGEN_PRESENT) {
    if (!(f & MON_LASTGEN_EQUAL)) {  // the generation is not synced yet
      lu = now;
      if (lssg) lu = ss - 10 * MON_MS;
    } else {
      if (lssg && lu > ss) lu = ss - 10 * MON_MS;
      update = false;
    }
  }
  uint8_t bits = update ? MON_UPDATE_ANNOTATION : (uint8_t)0;
  uint8_t result = MON_ALL_OK;
  // the first meters.Store, :207
  const int64_t st_lst = lst, st_oos = oos;
  bool stored = false;
  // ---- the status half, :210-251
  if ((f & MON_STATUS_ENABLED) && !(f & MON_STATUS_ABSENT)) {
    if (f & MON_FED_MISSING) {
      bits |= MON_MISSING_OG;
    } else if (f & MON_CLUSTER_ERR) {
      result = MON_STATUS_ERROR;
    } else if (!(f & MON_HAS_LAST)) {  // :313-317
      lst = now;
      bits |= MON_LOG_LAST_CLUSTER;
      stored = true;
    } else if (eq_cf) {  // synced, :319-323
      oos = 0;
      lst = now;
      bits |= MON_LOG_LAST_CLUSTER;
      stored = true;
    } else {  // out of sync, :324-340: the local meter changes and is not stored
      if (eq_lc) {
        oos = mon_sub(now, lst);
      } else {
        if (oos == 0) {
          oos = MON_SECOND;
          lst = now;
        } else {
          oos = mon_sub(now, lst);
        }
        bits |= MON_LOG_LAST_CLUSTER;
      }
      result = MON_REQUEUE;
    }
  }
  would[0] = lst;
  would[1] = oos;
  if (stored) bits |= MON_STATUS_STORED | MON_REPLACE_LAST;
  const int64_t w_lst = stored ? lst : st_lst, w_oos = stored ? oos : st_oos;
  d.t.col[MON_CR][slot] = cr;
  d.t.col[MON_LU][slot] = lu;
  d.t.col[MON_SS][slot] = ss;
  d.t.col[MON_LST][slot] = w_lst;
  d.t.col[MON_OOS][slot] = w_oos;
  d.t.type_id[slot] = d.type_id[o];
  d.t.flags[slot] = MON_LIVE;
  meter[MON_CR] = cr;
  meter[MON_LU] = lu;
  meter[MON_SS] = ss;
  meter[MON_LST] = w_lst;
  meter[MON_OOS] = w_oos;
  d.result[o] = result;
  d.bits[o] = bits;
}

}  // namespace

template <int W>
__global__ __launch_bounds__(MON_THREADS) void monitor_reconcile_kernel(MonRecDev d) {
  if ((int)blockIdx.x < d.n_long) {  // ---- long path: one listed object per block
    mon_object<256>(d, d.long_list[blockIdx.x], (int)threadIdx.x);
    return;
  }
  // ---- group path: groups past O, and those whose object is long, idle
  constexpr int GPB = MON_THREADS / W;
  const int gl = (int)threadIdx.x & (W - 1), g = (int)threadIdx.x / W;
  const int64_t stride = (int64_t)(gridDim.x - d.n_long) * GPB;
  for (int64_t base = (int64_t)(blockIdx.x - d.n_long) * GPB; base < d.O; base += stride) {
    const int64_t o = base + g;
    if (o < d.O && !d.obj_long[o]) mon_object<W>(d, (int)o, gl);
  }
}

// ------------------------------------------------------------------------------------------------ the report
namespace {

__device__ __forceinline__ void mon_add(int32_t* p, int v) { __hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void mon_lds_add(int32_t* p, int v) { __hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }

// a lane's MON_VEC consecutive slots of every column: 16-B loads (the table is allocated in whole block tiles and the
// columns start on 256 B, so slot i0, a multiple of MON_VEC, is aligned for each of them)
struct MonChunk {
  int64_t v[MON_COLS][MON_VEC];
  int32_t ty[MON_VEC];
  uint32_t fl;  // four flag bytes
};
template <bool TYPES>
__device__ __forceinline__ void mon_load(const MonTableDev& t, int64_t i0, MonChunk& c) {
#pragma unroll
  for (int k = 0; k < MON_COLS; ++k) {
    const longlong2* p = reinterpret_cast<const longlong2*>(t.col[k] + i0);
    const longlong2 a = p[0], b = p[1];
    c.v[k][0] = a.x;
    c.v[k][1] = a.y;
    c.v[k][2] = b.x;
    c.v[k][3] = b.y;
  }
  if (TYPES) {
    const int4 ty = *reinterpret_cast<const int4*>(t.type_id + i0);
    c.ty[0] = ty.x;
    c.ty[1] = ty.y;
    c.ty[2] = ty.z;
    c.ty[3] = ty.w;
  }
  c.fl = *reinterpret_cast<const uint32_t*>(t.flags + i0);
}

// what report.go does with one meter
struct MonEval {
  bool late;     // start.After(syncSuccessTimestamp): the object has not been synced (report.go:112)
  bool t_sync;   // a totalsync.latency.ms timer (:67-78)
  bool t_stat;   // a totalstatus.latency.ms timer (:46-54)
  int64_t start, sync_ms, stat_ms;
};
__device__ __forceinline__ MonEval mon_eval(const MonChunk& c, int j, bool live, int64_t now) {
  MonEval e;
  const int64_t cr = c.v[MON_CR][j], lu = c.v[MON_LU][j], ss = c.v[MON_SS][j], lst = c.v[MON_LST][j], oos = c.v[MON_OOS][j];
  e.start = lu > cr ? lu : cr;  // :68-71, :101-104
  e.late = live && e.start > ss;
  e.t_sync = live && ss + MON_REPORT_INTERVAL > now && ss > e.start;
  e.sync_ms = mon_sub(ss, e.start) / MON_MS;  // Duration.Milliseconds truncates
  e.t_stat = live && lst != MON_ZERO && oos > MON_REPORT_INTERVAL;
  e.stat_ms = oos / MON_MS;
  return e;
}
__device__ __forceinline__ bool mon_live(const MonChunk& c, int j, int64_t i, int64_t n) {
  return i < n && ((c.fl >> (8 * j)) & MON_LIVE);
}

__constant__ const int64_t MON_BUCKET_NS[MON_BUCKETS] = {5 * MON_MINUTE,  10 * MON_MINUTE,  30 * MON_MINUTE,
                                                        60 * MON_MINUTE, 180 * MON_MINUTE, 1440 * MON_MINUTE};

}  // namespace

template <int PATH>
__global__ __launch_bounds__(MON_THREADS) void monitor_scan_kernel(MonRepDev d) {
  extern __shared__ int32_t mon_lds[];  // [16] the block's counters, then (LDS path) [2 * n_types] bins
  int32_t* const s_cnt = mon_lds;
  int32_t* const bins = mon_lds + 16;
  const int nb = PATH == MON_PATH_LDS ? 2 * d.n_types : 0;
  for (int i = threadIdx.x; i < 16 + nb; i += MON_THREADS) mon_lds[i] = 0;
  __syncthreads();
  int32_t* const h_sync = PATH == MON_PATH_LDS ? bins : d.hist;
  int32_t* const h_stat = h_sync + d.n_types;
  int wc[MON_COUNTERS];  // wave-uniform
#pragma unroll
  for (int k = 0; k < MON_COUNTERS; ++k) wc[k] = 0;
  const int lane = lane_id_h(), wave = (int)threadIdx.x >> 6;
  const int64_t n = d.n_slots, now = d.now;
  // the trip count is the same for every lane of a block: a block tile is read whole (the table ends on one)
  for (int64_t tile = blockIdx.x; tile * MON_BTILE < n; tile += gridDim.x) {
    const int64_t i0 = tile * MON_BTILE + (int64_t)threadIdx.x * MON_VEC;
    MonChunk c;
    mon_load<true>(d.t, i0, c);
    int n_sync = 0, n_stat = 0;
    MonEval e[MON_VEC];
    bool any_late = false;
#pragma unroll
    for (int j = 0; j < MON_VEC; ++j) {
      e[j] = mon_eval(c, j, mon_live(c, j, i0 + j, n), now);
      n_sync += e[j].t_sync;
      n_stat += e[j].t_stat;
      any_late |= e[j].late;
      wc[12] += popc64(ballot(e[j].t_sync));
      wc[13] += popc64(ballot(e[j].t_stat));
    }
    if (ballot(any_late)) {  // wave-uniform: most tables hold synced objects only
#pragma unroll
      for (int j = 0; j < MON_VEC; ++j) {
        const int64_t oos = c.v[MON_OOS][j];
#pragma unroll
        for (int b = 0; b < MON_BUCKETS; ++b) {
          const bool s = e[j].late && now > e[j].start + MON_BUCKET_NS[b];  // :114
          const bool t = e[j].late && oos > MON_BUCKET_NS[b];               // :128
          wc[b] += popc64(ballot(s));
          wc[MON_BUCKETS + b] += popc64(ballot(t));
          if (b == 0) {  // :124-126, :137-139
            if (s) (PATH == MON_PATH_LDS) ? mon_lds_add(h_sync + c.ty[j], 1) : mon_add(h_sync + c.ty[j], 1);
            if (t) (PATH == MON_PATH_LDS) ? mon_lds_add(h_stat + c.ty[j], 1) : mon_add(h_stat + c.ty[j], 1);
          }
        }
      }
    }
    // this wave's tile of the timer lists' counts
    const int ts = wave_sum_u_i32(n_sync | (n_stat << 16));
    const int64_t wt = tile * (MON_BTILE / MON_WTILE) + wave;
    if (lane == 0 && wt < d.n_wtiles) d.tile_cnt[wt] = ts;
  }
  if (lane == 0) {
#pragma unroll
    for (int k = 0; k < MON_COUNTERS; ++k)
      if (wc[k]) mon_lds_add(s_cnt + k, wc[k]);
  }
  __syncthreads();
  if (threadIdx.x < MON_COUNTERS && s_cnt[threadIdx.x]) mon_add(d.counters + threadIdx.x, s_cnt[threadIdx.x]);
  if (PATH == MON_PATH_LDS)
    for (int i = threadIdx.x; i < nb; i += MON_THREADS) {
      const int v = bins[i];
      if (v) mon_add(d.hist + i, v);
    }
}

// one wave: tile_off[0][t], tile_off[1][t] = the timers of the tiles below t, n_timers = the totals
__global__ __launch_bounds__(64) void monitor_offsets_kernel(MonRepDev d) {
  const int lane = lane_id_h(), T = d.n_wtiles;
  int32_t* const off_sync = d.tile_off;
  int32_t* const off_stat = d.tile_off + (T + 1);
  int carry_s = 0, carry_t = 0;
  for (int base = 0; base < T; base += WAVE) {
    const int t = base + lane;
    const int v = t < T ? d.tile_cnt[t] : 0;
    const int vs = v & 0xffff, vt = (int)((uint32_t)v >> 16);
    const int is = wave_incl_sum_i32(vs), it = wave_incl_sum_i32(vt);
    if (t < T) {
      off_sync[t] = carry_s + is - vs;
      off_stat[t] = carry_t + it - vt;
    }
    carry_s += __builtin_amdgcn_readlane(is, 63);
    carry_t += __builtin_amdgcn_readlane(it, 63);
  }
  if (lane == 0) {
    off_sync[T] = carry_s;
    off_stat[T] = carry_t;
    d.n_timers[0] = carry_s;
    d.n_timers[1] = carry_t;
  }
}

__global__ __launch_bounds__(MON_THREADS) void monitor_scatter_kernel(MonRepDev d) {
  const int lane = lane_id_h(), wave = (int)threadIdx.x >> 6, T = d.n_wtiles;
  const int32_t* const off_sync = d.tile_off;
  const int32_t* const off_stat = d.tile_off + (T + 1);
  const int64_t n = d.n_slots, now = d.now;
  for (int64_t tile = blockIdx.x; tile * MON_BTILE < n; tile += gridDim.x) {
    const int64_t wt = tile * (MON_BTILE / MON_WTILE) + wave;
    if (wt >= T) continue;  // wave-uniform
    const int at_s = off_sync[wt], at_t = off_stat[wt];
    if (off_sync[wt + 1] == at_s && off_stat[wt + 1] == at_t) continue;  // wave-uniform: no timer in this tile
    const int64_t i0 = wt * MON_WTILE + (int64_t)lane * MON_VEC;
    MonChunk c;
    mon_load<false>(d.t, i0, c);
    MonEval e[MON_VEC];
    int n_sync = 0, n_stat = 0;
#pragma unroll
    for (int j = 0; j < MON_VEC; ++j) {
      e[j] = mon_eval(c, j, mon_live(c, j, i0 + j, n), now);
      n_sync += e[j].t_sync;
      n_stat += e[j].t_stat;
    }
    // a lane's slots ascend and so do the lanes': an entry's place is the entries of the lanes below plus its own
    int ps = at_s + wave_incl_sum_i32(n_sync) - n_sync, pt = at_t + wave_incl_sum_i32(n_stat) - n_stat;
#pragma unroll
    for (int j = 0; j < MON_VEC; ++j) {
      if (e[j].t_sync) {
        if (ps < d.timer_cap) {
          d.sync_slot[ps] = (int32_t)(i0 + j);
          d.sync_ms[ps] = e[j].sync_ms;
        }
        ++ps;
      }
      if (e[j].t_stat) {
        if (pt < d.timer_cap) {
          d.status_slot[pt] = (int32_t)(i0 + j);
          d.status_ms[pt] = e[j].stat_ms;
        }
        ++pt;
      }
    }
  }
}

template <bool LOAD>
__global__ __launch_bounds__(MON_THREADS) void monitor_io_kernel(MonIoDev d) {
  const int i = blockIdx.x * MON_THREADS + threadIdx.x;
  if (i >= d.n) return;
  const int64_t s = d.slots[i];
#pragma unroll
  for (int k = 0; k < MON_COLS; ++k)
    if (d.col[k]) {
      if (LOAD)
        d.t.col[k][s] = d.col[k][i];
      else
        d.col[k][i] = d.t.col[k][s];
    }
  if (d.type_id) {
    if (LOAD)
      d.t.type_id[s] = d.type_id[i];
    else
      d.type_id[i] = d.t.type_id[s];
  }
  if (d.flags) {
    if (LOAD)
      d.t.flags[s] = d.flags[i];
    else
      d.flags[i] = d.t.flags[s];
  }
}

hipError_t launch_monitor_reconcile(const MonRecDev& d, const MonRecRoute& r, hipStream_t st) {
  (void)hipGetLastError();
  const unsigned grid = (unsigned)(r.grid + r.long_grid);
  if (grid > 0)
    with_width<1>(r.width, [&](auto W) {
      hipLaunchKernelGGL((monitor_reconcile_kernel<decltype(W)::value>), dim3(grid), dim3(MON_THREADS), 0, st, d);
    });
  return hipGetLastError();
}

hipError_t launch_monitor_report(const MonRepDev& d, const MonRepRoute& r, hipStream_t st) {
  (void)hipGetLastError();
  if (r.grid > 0) {
    if (r.path == MON_PATH_LDS)
      hipLaunchKernelGGL(monitor_scan_kernel<MON_PATH_LDS>, dim3((unsigned)r.grid), dim3(MON_THREADS),
                         (size_t)(16 + 2 * d.n_types) * sizeof(int32_t), st, d);
    else
      hipLaunchKernelGGL(monitor_scan_kernel<MON_PATH_GLOBAL>, dim3((unsigned)r.grid), dim3(MON_THREADS), 16 * sizeof(int32_t), st, d);
  }
  return hipGetLastError();
}

hipError_t launch_monitor_timers(const MonRepDev& d, const MonRepRoute& r, hipStream_t st) {
  (void)hipGetLastError();
  hipLaunchKernelGGL(monitor_offsets_kernel, dim3(1), dim3(64), 0, st, d);
  if (r.grid > 0) hipLaunchKernelGGL(monitor_scatter_kernel, dim3((unsigned)r.grid), dim3(MON_THREADS), 0, st, d);
  return hipGetLastError();
}

hipError_t launch_monitor_io(const MonIoDev& d, bool load, hipStream_t st) {
  (void)hipGetLastError();
  const unsigned grid = (unsigned)((d.n + MON_THREADS - 1) / MON_THREADS);
  if (grid > 0) {
    if (load)
      hipLaunchKernelGGL(monitor_io_kernel<true>, dim3(grid), dim3(MON_THREADS), 0, st, d);
    else
      hipLaunchKernelGGL(monitor_io_kernel<false>, dim3(grid), dim3(MON_THREADS), 0, st, d);
  }
  return hipGetLastError();
}

}  // namespace kad

// ------------------------------------------------------ host half: kad_monitor_*
#include "kad_arena.h"

using namespace kad;

namespace {

MonTableDev table_dev(kad_ctx* c) {
  MonTableDev t{};
  for (int k = 0; k < MON_COLS; ++k) t.col[k] = c->mon.col[k].as<int64_t>();
  t.type_id = c->mon.type_id.as<int32_t>();
  t.flags = c->mon.flags.as<uint8_t>();
  return t;
}

// a time the table may hold: real, or within 2^60 of the zero time
inline bool time_ok(int64_t t) { return (t >= 0 && t < MON_TIME_END) || (t >= MON_ZERO - (1ll << 60) && t <= MON_ZERO + (1ll << 60)); }
inline bool real_or_zero(int64_t t) { return (t >= 0 && t < MON_TIME_END) || t == MON_ZERO; }

// grows the table to hold `capacity` slots, in whole block tiles, zeroed; the contents stay
int reserve_locked(kad_ctx* c, int64_t capacity) {
  MonTable& m = c->mon;
  if (capacity <= m.cap) return KAD_OK;
  if (capacity > INT32_MAX - MON_BTILE) return fail(c, KAD_EUNSUPPORTED, "kad_monitor_reserve: more than 2^31 - 1 slots");
  HIPCHK(c, hipSetDevice(c->device));
  const int64_t cap = (capacity + MON_BTILE - 1) / MON_BTILE * MON_BTILE;
  DevBuf fresh[MON_COLS + 2];
  const size_t width[MON_COLS + 2] = {8, 8, 8, 8, 8, 4, 1};
  DevBuf* old[MON_COLS + 2] = {&m.col[0], &m.col[1], &m.col[2], &m.col[3], &m.col[4], &m.type_id, &m.flags};
  for (int k = 0; k < MON_COLS + 2; ++k) {
    if (int r = grow(c, fresh[k], (size_t)cap * width[k])) return r;
    HIPCHK(c, hipMemsetAsync(fresh[k].p, 0, (size_t)cap * width[k], c->stream));
    if (m.cap) HIPCHK(c, hipMemcpyAsync(fresh[k].p, old[k]->p, (size_t)m.cap * width[k], hipMemcpyDeviceToDevice, c->stream));
  }
  HIPCHK(c, hipStreamSynchronize(c->stream));
  for (int k = 0; k < MON_COLS + 2; ++k) {
    std::swap(fresh[k].p, old[k]->p);
    std::swap(fresh[k].cap, old[k]->cap);
  }
  m.live.resize((size_t)cap, 0);
  m.cap = cap;
  return KAD_OK;
}

// n distinct slots in [0, cap): the shadow's high bit marks the slots seen so far
int slots_check(kad_ctx* c, int64_t n, const int32_t* slots, const char* who) {
  const int64_t cap = c->mon.cap;
  if (n && !slots) return fail(c, KAD_EINVAL, std::string(who) + ": slots missing");
  if (first_bad(n, [=](int64_t i) { return slots[i] < 0; }) >= 0) return fail(c, KAD_EINVAL, std::string(who) + ": negative slot");
  if (first_bad(n, [=](int64_t i) { return slots[i] >= cap; }) >= 0)
    return fail(c, KAD_ENOSPC, std::string(who) + ": a slot at or beyond the table's capacity (kad_monitor_reserve)");
  std::vector<uint8_t>& live = c->mon.live;
  int64_t dup = -1;
  for (int64_t i = 0; i < n && dup < 0; ++i) {
    uint8_t& v = live[(size_t)slots[i]];
    if (v & 0x80) dup = i;
    v |= 0x80;
  }
  for (int64_t i = 0; i < n; ++i) live[(size_t)slots[i]] &= 0x7f;
  if (dup >= 0) return fail(c, KAD_EINVAL, std::string(who) + ": a slot is listed twice");
  return KAD_OK;
}

struct RecPlan {
  std::vector<uint8_t> obj_long;
  std::vector<int32_t> long_list;
  int64_t short_items = 0;
};

// a CSR of O rows of (cluster id in [0, C), generation), strictly ascending by cluster within a row
inline bool list_bad(const int32_t* off, const int32_t* cl, const int64_t* gen, int64_t O, int64_t C) {
  if (csr_bad(off, cl, O, 0, C)) return true;
  if (off[O] && !gen) return true;
  return first_bad(O, [=](int64_t i) {
           for (int64_t k = (int64_t)off[i] + 1; k < off[i + 1]; ++k)
             if (cl[k] <= cl[k - 1]) return true;
           return false;
         }) >= 0;
}

int validate_reconcile(const kad_monitor_batch* b, const kad_monitor_view* out, int long_min, RecPlan* plan, std::string* err) {
  auto bad = [&](const char* m) {
    *err = m;
    return KAD_EINVAL;
  };
  const int64_t O = b->n_objects, C = b->n_clusters;
  if (O < 0 || C < 0) return bad("negative count");
  if (C > MON_MAX_CLUSTERS) {
    *err = "more than KAD_DISPATCH_MAX_CLUSTERS clusters";
    return KAD_EUNSUPPORTED;
  }
  if (b->now_ns < 0 || b->now_ns >= MON_TIME_END) return bad("now_ns outside [0, 2^62)");
  if (O && (!b->slot || !b->obj_flags || !b->type_id || !b->creation_ns || !b->sync_success_ns)) return bad("input array missing");
  if (list_bad(b->fed_off, b->fed_cluster, b->fed_gen, O, C)) return bad("fed malformed, id outside [0, n_clusters) or not strictly ascending");
  if (list_bad(b->mem_off, b->mem_cluster, b->mem_gen, O, C)) return bad("mem malformed, id outside [0, n_clusters) or not strictly ascending");
  if (list_bad(b->last_off, b->last_cluster, b->last_gen, O, C)) return bad("last malformed, id outside [0, n_clusters) or not strictly ascending");
  const uint16_t* of = b->obj_flags;
  const int32_t *ty = b->type_id, *lo = b->last_off;
  const int64_t *cr = b->creation_ns, *ss = b->sync_success_ns;
  if (first_bad(O, [=](int64_t i) {
        const uint16_t f = of[i];
        if ((f & ~MON_OBJ_ALL) || ty[i] < 0) return true;
        if ((f & MON_NEW) && ((f & MON_HAS_LAST) || !real_or_zero(cr[i]))) return true;
        if ((f & MON_SS_PARSED) && !real_or_zero(ss[i])) return true;
        if (!(f & MON_HAS_LAST) && lo[i + 1] != lo[i]) return true;
        return false;
      }) >= 0)
    return bad("obj_flags: unknown or inconsistent flag, a negative type_id, a time outside its range, or a last list without HAS_LAST");
  if (!out || (O && (!out->result || !out->bits || !out->meter || !out->would))) return bad("output view missing");
  if (plan) {
    const int32_t *fo = b->fed_off, *mo = b->mem_off;
    plan->obj_long.assign((size_t)O, 0);
    for (int64_t i = 0; i < O; ++i) {
      const int64_t n = std::max<int64_t>({fo[i + 1] - fo[i], mo[i + 1] - mo[i], lo[i + 1] - lo[i]});
      if (n <= long_min) {
        plan->short_items += n;
        continue;
      }
      plan->obj_long[(size_t)i] = 1;
      plan->long_list.push_back((int32_t)i);
    }
  }
  return KAD_OK;
}

int reconcile_locked(kad_ctx* c, const kad_monitor_batch* b, const kad_monitor_view* out) {
  Stage& stg = c->stage[STG_MONREC];
  const int long_min = stg.force.long_min_or(MON_LONG_MIN);
  std::string err;
  RecPlan plan;
  if (int r = validate_reconcile(b, out, long_min, &plan, &err)) return fail(c, r, err);
  const int O = b->n_objects;
  if (O == 0) return KAD_OK;
  if (int r = slots_check(c, O, b->slot, "kad_monitor_reconcile")) return r;
  MonTable& m = c->mon;
  const int32_t* sl = b->slot;
  const uint16_t* of = b->obj_flags;
  for (int i = 0; i < O; ++i) {  // NEW agrees with the slot's LIVE flag
    const bool live = m.live[(size_t)sl[i]] != 0;
    if (!(of[i] & MON_DELETED) && live == ((of[i] & MON_NEW) != 0))
      return fail(c, KAD_EINVAL, "kad_monitor_reconcile: KAD_MON_OBJ_NEW on a live slot, or a dead slot without it");
  }
  HIPCHK(c, hipSetDevice(c->device));
  const int n_long = (int)plan.long_list.size();
  MonRecRoute route = route_monitor_reconcile(O, n_long, plan.short_items, n_cus());
  group_force_apply(stg.force, n_long < O, O, n_cus(), route.width, route.grid, &route.stride);
  route.long_min = long_min;
  const size_t o = (size_t)O, nf = (size_t)b->fed_off[O], nm = (size_t)b->mem_off[O], nl = (size_t)b->last_off[O];
  MonRecDev d{};
  d.O = O;
  d.n_long = n_long;
  d.now = b->now_ns;
  d.t = table_dev(c);
  Arena a;
  a.in(d.slot, b->slot, o);
  a.in(d.obj_flags, b->obj_flags, o);
  a.in(d.type_id, b->type_id, o);
  a.in(d.creation, b->creation_ns, o);
  a.in(d.sync_success, b->sync_success_ns, o);
  a.in(d.fed.off, b->fed_off, o + 1);
  a.in(d.fed.cluster, b->fed_cluster, nf);
  a.in(d.fed.gen, b->fed_gen, nf);
  a.in(d.mem.off, b->mem_off, o + 1);
  a.in(d.mem.cluster, b->mem_cluster, nm);
  a.in(d.mem.gen, b->mem_gen, nm);
  a.in(d.last.off, b->last_off, o + 1);
  a.in(d.last.cluster, b->last_cluster, nl);
  a.in(d.last.gen, b->last_gen, nl);
  a.in(d.obj_long, plan.obj_long.data(), o);
  a.in(d.long_list, plan.long_list.data(), (size_t)n_long);
  a.out(d.result, out->result, o);
  a.out(d.bits, out->bits, o);
  a.out(d.meter, out->meter, o * MON_COLS);
  a.out(d.would, out->would, o * 2);
  HIPCHK(c, hipEventRecord(stg.ev[0], c->stream));
  if (int r = a.commit(c, stg.buf)) return r;
  HIPCHK(c, hipEventRecord(stg.ev[1], c->stream));
  HIPCHK(c, launch_monitor_reconcile(d, route, c->stream));
  HIPCHK(c, hipEventRecord(stg.ev[2], c->stream));
  if (int r = a.fetch(c)) return r;
  HIPCHK(c, hipEventRecord(stg.ev[3], c->stream));
  stage_ran(stg, route);
  HIPCHK(c, hipStreamSynchronize(c->stream));
  for (int i = 0; i < O; ++i) {  // the host's shadow follows the kernel
    uint8_t& lv = m.live[(size_t)sl[i]];
    const bool del = (of[i] & MON_DELETED) != 0;
    m.n_live += (del ? 0 : 1) - (lv ? 1 : 0);
    lv = del ? 0 : 1;
    if (!del) {
      m.n_slots = std::max<int64_t>(m.n_slots, (int64_t)sl[i] + 1);
      m.max_type = std::max(m.max_type, b->type_id[i]);
    }
  }
  return KAD_OK;
}

int validate_report(const kad_monitor_report_batch* b, const kad_monitor_report_view* out, std::string* err) {
  auto bad = [&](const char* m) {
    *err = m;
    return KAD_EINVAL;
  };
  if (b->now_ns < 0 || b->now_ns >= MON_TIME_END) return bad("now_ns outside [0, 2^62)");
  if (b->n_types < 0 || b->timer_cap < 0) return bad("negative count");
  if (!out || !out->counters || !out->n_timers || (b->n_types && (!out->type_sync || !out->type_status)) ||
      (b->timer_cap && (!out->sync_slot || !out->sync_ms || !out->status_slot || !out->status_ms)))
    return bad("output view missing");
  return KAD_OK;
}

int report_locked(kad_ctx* c, const kad_monitor_report_batch* b, const kad_monitor_report_view* out) {
  std::string err;
  if (int r = validate_report(b, out, &err)) return fail(c, r, err);
  MonTable& m = c->mon;
  Stage& stg = c->stage[STG_MONREP];
  if (b->n_types <= m.max_type) return fail(c, KAD_EINVAL, "kad_monitor_report: n_types does not exceed every stored type id");
  if (stg.force.path == 1 && b->n_types > MON_LDS_TYPES)
    return fail(c, KAD_EINVAL, "kad_monitor_report_debug_route: the LDS-private path forced on more types than its bins");
  HIPCHK(c, hipSetDevice(c->device));
  const MonRepRoute route = route_monitor_report(m.n_slots, b->n_types, n_cus(), stg.force.path, stg.force.grid);
  const size_t nt = (size_t)b->n_types, cap = (size_t)b->timer_cap, T = (size_t)route.wtiles;
  MonRepDev d{};
  d.n_slots = m.n_slots;
  d.now = b->now_ns;
  d.n_types = b->n_types;
  d.n_wtiles = route.wtiles;
  d.timer_cap = b->timer_cap;
  d.t = table_dev(c);
  Arena a;
  a.out(d.counters, out->counters, MON_COUNTERS);
  a.out(d.n_timers, out->n_timers, 2);
  a.out(d.tile_cnt, T);
  a.out(d.tile_off, 2 * (T + 1));
  a.out(d.sync_slot, out->sync_slot, cap);
  a.out(d.sync_ms, out->sync_ms, cap);
  a.out(d.status_slot, out->status_slot, cap);
  a.out(d.status_ms, out->status_ms, cap);
  a.out(d.hist, 2 * nt);
  HIPCHK(c, hipEventRecord(stg.ev[0], c->stream));
  if (int r = a.commit(c, stg.buf)) return r;
  HIPCHK(c, hipMemsetAsync(d.counters, 0, MON_COUNTERS * sizeof(int32_t), c->stream));
  HIPCHK(c, hipMemsetAsync(d.hist, 0, std::max<size_t>(1, 2 * nt) * sizeof(int32_t), c->stream));
  if (T) HIPCHK(c, hipMemsetAsync(d.tile_cnt, 0, T * sizeof(int32_t), c->stream));
  HIPCHK(c, hipEventRecord(stg.ev[1], c->stream));
  HIPCHK(c, launch_monitor_report(d, route, c->stream));
  HIPCHK(c, hipEventRecord(stg.ev[2], c->stream));
  HIPCHK(c, launch_monitor_timers(d, route, c->stream));
  HIPCHK(c, hipEventRecord(stg.ev[3], c->stream));
  if (int r = a.fetch(c)) return r;
  if (nt) {
    HIPCHK(c, hipMemcpyAsync(out->type_sync, d.hist, nt * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(out->type_status, d.hist + nt, nt * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
  }
  stage_ran(stg, route);
  HIPCHK(c, hipStreamSynchronize(c->stream));
  if (out->n_timers[0] > b->timer_cap || out->n_timers[1] > b->timer_cap)
    return fail(c, KAD_ENOSPC, "kad_monitor_report: a timer list is longer than timer_cap (n_timers holds the lengths)");
  return KAD_OK;
}

// kad_monitor_load (load) / kad_monitor_read: the listed slots of the given columns
int io_locked(kad_ctx* c, bool load, int32_t n, const int32_t* slots, int64_t* const cols[MON_COLS], int32_t* type_id, uint8_t* flags) {
  const char* who = load ? "kad_monitor_load" : "kad_monitor_read";
  if (n < 0) return fail(c, KAD_EINVAL, std::string(who) + ": negative count");
  if (n == 0) return KAD_OK;
  if (int r = slots_check(c, n, slots, who)) return r;
  MonTable& m = c->mon;
  if (load) {
    for (int k = 0; k < MON_COLS; ++k) {
      const int64_t* v = cols[k];
      if (!v) continue;
      const bool dur = k == MON_OOS;
      if (first_bad(n, [=](int64_t i) { return dur ? false : !time_ok(v[i]); }) >= 0)
        return fail(c, KAD_EINVAL, "kad_monitor_load: a time that is neither real nor within 2^60 of KAD_MON_TIME_ZERO");
    }
    if (type_id && first_bad(n, [=](int64_t i) { return type_id[i] < 0; }) >= 0) return fail(c, KAD_EINVAL, "kad_monitor_load: negative type_id");
    if (flags && first_bad(n, [=](int64_t i) { return (flags[i] & ~MON_LIVE) != 0; }) >= 0) return fail(c, KAD_EINVAL, "kad_monitor_load: unknown flag");
    if (flags && !type_id) return fail(c, KAD_EINVAL, "kad_monitor_load: flags without type_id (a live slot's type must be known)");
  }
  HIPCHK(c, hipSetDevice(c->device));
  Stage& stg = c->stage[STG_MONIO];
  MonIoDev d{};
  d.n = n;
  d.t = table_dev(c);
  Arena a;
  a.in(d.slots, slots, (size_t)n);
  for (int k = 0; k < MON_COLS; ++k) {
    if (!cols[k])
      Arena::absent(d.col[k]);
    else if (load)
      a.in(const_cast<const int64_t*&>(d.col[k]), const_cast<const int64_t*>(cols[k]), (size_t)n);
    else
      a.out(d.col[k], cols[k], (size_t)n);
  }
  if (!type_id)
    Arena::absent(d.type_id);
  else if (load)
    a.in(const_cast<const int32_t*&>(d.type_id), const_cast<const int32_t*>(type_id), (size_t)n);
  else
    a.out(d.type_id, type_id, (size_t)n);
  if (!flags)
    Arena::absent(d.flags);
  else if (load)
    a.in(const_cast<const uint8_t*&>(d.flags), const_cast<const uint8_t*>(flags), (size_t)n);
  else
    a.out(d.flags, flags, (size_t)n);
  if (int r = a.commit(c, stg.buf)) return r;
  HIPCHK(c, launch_monitor_io(d, load, c->stream));
  if (int r = a.fetch(c)) return r;
  HIPCHK(c, hipStreamSynchronize(c->stream));
  if (load)
    for (int i = 0; i < n; ++i) {
      m.n_slots = std::max<int64_t>(m.n_slots, (int64_t)slots[i] + 1);
      if (type_id) m.max_type = std::max(m.max_type, type_id[i]);
      if (flags) {
        uint8_t& lv = m.live[(size_t)slots[i]];
        const uint8_t nv = flags[i] & MON_LIVE;
        m.n_live += (int)nv - (int)lv;
        lv = nv;
      }
    }
  return KAD_OK;
}

}  // namespace

extern "C" {

int kad_monitor_reserve(kad_ctx* c, int64_t capacity) {
  return entry(c, capacity >= 0, [&]() -> int {
    return reserve_locked(c, capacity);
  });
}

int kad_monitor_load(kad_ctx* c, int32_t n, const int32_t* slots, const int64_t* creation, const int64_t* last_update,
                     const int64_t* sync_success, const int64_t* last_status_synced, const int64_t* out_of_sync_ns,
                     const int32_t* type_id, const uint8_t* flags) {
  return entry(c, true, [&]() -> int {
    int64_t* const cols[MON_COLS] = {const_cast<int64_t*>(creation), const_cast<int64_t*>(last_update), const_cast<int64_t*>(sync_success),
                                     const_cast<int64_t*>(last_status_synced), const_cast<int64_t*>(out_of_sync_ns)};
    return io_locked(c, true, n, slots, cols, const_cast<int32_t*>(type_id), const_cast<uint8_t*>(flags));
  });
}

int kad_monitor_read(kad_ctx* c, int32_t n, const int32_t* slots, int64_t* creation, int64_t* last_update, int64_t* sync_success,
                     int64_t* last_status_synced, int64_t* out_of_sync_ns, int32_t* type_id, uint8_t* flags) {
  return entry(c, true, [&]() -> int {
    int64_t* const cols[MON_COLS] = {creation, last_update, sync_success, last_status_synced, out_of_sync_ns};
    return io_locked(c, false, n, slots, cols, type_id, flags);
  });
}

int kad_monitor_clear(kad_ctx* c) {
  return entry(c, true, [&]() -> int {
    MonTable& m = c->mon;
    if (m.cap) {
      HIPCHK(c, hipSetDevice(c->device));
      HIPCHK(c, hipMemsetAsync(m.flags.p, 0, (size_t)m.cap, c->stream));
      HIPCHK(c, hipStreamSynchronize(c->stream));
    }
    std::fill(m.live.begin(), m.live.end(), (uint8_t)0);
    m.n_slots = m.n_live = 0;
    m.max_type = -1;
    return KAD_OK;
  });
}

int kad_monitor_info(kad_ctx* c, int64_t out[4]) {
  return entry(c, out != nullptr, [&]() -> int {
    out[0] = c->mon.cap;
    out[1] = c->mon.n_slots;
    out[2] = c->mon.n_live;
    out[3] = c->mon.max_type;
    return KAD_OK;
  });
}

int kad_monitor_reconcile_check(const kad_monitor_batch* b, const kad_monitor_view* out) {
  return check_guarded([&]() -> int {
    if (!b) return KAD_EINVAL;
    std::string err;
    return validate_reconcile(b, out, MON_LONG_MIN, nullptr, &err);
  });
}

int kad_monitor_reconcile(kad_ctx* c, const kad_monitor_batch* b, const kad_monitor_view* out) {
  return entry(c, b != nullptr, [&]() -> int {
    return reconcile_locked(c, b, out);
  });
}

int kad_monitor_reconcile_timing(kad_ctx* c, float ms[3]) { return stage_timing(c, STG_MONREC, 3, ms, "no kad_monitor_reconcile ran"); }

int kad_monitor_reconcile_route_eval(int32_t n_objects, int32_t n_long, int64_t short_items, int32_t n_cu, int32_t* out) {
  if (!out || n_objects < 0 || n_long < 0 || n_long > n_objects || short_items < 0 || n_cu < 1) return KAD_EINVAL;
  return route_record<KAD_MON_REC_ROUTE_FIELDS>(out, route_monitor_reconcile(n_objects, n_long, short_items, n_cu));
}

int kad_monitor_reconcile_last_route(kad_ctx* c, int32_t* out) {
  return stage_last_route(c, STG_MONREC, out, "no kad_monitor_reconcile ran");
}

int kad_monitor_reconcile_debug_route(kad_ctx* c, int32_t force_width, int32_t force_long_min) {
  return stage_debug_route(c, STG_MONREC, group_width_ok(force_width, 1), GroupForce{force_width, force_long_min, 0});
}

int kad_monitor_report_check(const kad_monitor_report_batch* b, const kad_monitor_report_view* out) {
  return check_guarded([&]() -> int {
    if (!b) return KAD_EINVAL;
    std::string err;
    return validate_report(b, out, &err);
  });
}

int kad_monitor_report(kad_ctx* c, const kad_monitor_report_batch* b, const kad_monitor_report_view* out) {
  return entry(c, b != nullptr, [&]() -> int {
    return report_locked(c, b, out);
  });
}

int kad_monitor_report_timing(kad_ctx* c, float ms[3]) { return stage_timing(c, STG_MONREP, 3, ms, "no kad_monitor_report ran"); }

int kad_monitor_report_route_eval(int64_t n_slots, int32_t n_types, int32_t n_cu, int32_t* out) {
  if (!out || n_slots < 0 || n_slots > INT32_MAX || n_types < 0 || n_cu < 1) return KAD_EINVAL;
  return route_record<KAD_MON_REP_ROUTE_FIELDS>(out, route_monitor_report(n_slots, n_types, n_cu));
}

int kad_monitor_report_last_route(kad_ctx* c, int32_t* out) { return stage_last_route(c, STG_MONREP, out, "no kad_monitor_report ran"); }

int kad_monitor_report_debug_route(kad_ctx* c, int32_t force_path, int32_t force_grid) {
  return stage_debug_route(c, STG_MONREP, force_path >= 0 && force_path <= 2 && force_grid >= 0, GroupForce{0, 0, 0, force_path, force_grid});
}

}  // extern "C"
