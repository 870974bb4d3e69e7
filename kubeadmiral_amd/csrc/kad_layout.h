// LDS / scratch layouts and block shapes of the schedule kernels: read by the kernels for their offsets and
// by the host's route decision (kad_route.h) for the launch sizes. Plain arithmetic, no HIP calls: the file
// also compiles as host-only C++.
#pragma once
#include <stddef.h>
#include <stdint.h>

#ifdef __HIPCC__
#define KAD_HD __host__ __device__
#else
#define KAD_HD
#endif

namespace kad {

constexpr int WIDE_Q = 8;                       // schedule_wide_kernel: positions per lane
constexpr int WIDE_P = WIDE_Q * 64;             //   and per wave (longer feasible lists: schedule_row_kernel)
constexpr int LDS_BUDGET = 64 * 1024;           // per block, of the kernels that do not raise their LDS limit
constexpr int LDS_MAX = 160 * 1024;             // per block, of the wide and row kernels (gfx950: 160 KB per CU)

// ----------------------------------------------------------- per-wave layout
struct RowLayout {
  size_t tot, fx, idx, perm, posl, posr, feas, sel, place, cur, hist, bytes;
};
KAD_HD inline RowLayout row_layout(int C) {
  const size_t Cp = (size_t)((C + 63) & ~63);
  const size_t nw = Cp / 64;
  RowLayout L;
  L.tot = 0;                                     // i64[Cp] total per feasible position
  L.fx = L.tot + 8 * Cp;                         // u32[Cp] fixed scores | TT raw << 16
  L.idx = L.fx + 4 * Cp;                         // u16[Cp] feasible position → cluster id
  L.perm = L.idx + 2 * Cp;                       // u16[Cp] pdqsort replay permutation
  L.posl = L.perm + 2 * Cp;                      // u16[Cp] replay scratch (partition stoppers)
  L.posr = L.posl + 2 * Cp + 128;                // u16[Cp] (posl: Cp + 64 entries, PdqWave)
  L.feas = (L.posr + 2 * Cp + 15) & ~(size_t)15;  // u64[nw] feasibility by cluster
  L.sel = L.feas + 8 * nw;                       // u64[nw] selection by position
  L.place = L.sel + 8 * nw;
  L.cur = L.place + 8 * nw;
  L.hist = L.cur + 8 * nw;
  L.bytes = (L.hist + 4 * 256 + 15) & ~(size_t)15;
  return L;
}
// GSCR rows (state in a global slab): the small per-wave arrays that take atomics — selection, placement
// and current-cluster bitmaps, the radix histogram — stay in LDS (dynamic LDS of the 1-wave blocks)
struct SmallLayout {
  size_t sel, place, cur, hist, bytes;
};
KAD_HD inline SmallLayout small_layout(int C) {
  const size_t nw = (size_t)((C + 63) / 64);
  SmallLayout L;
  L.sel = 0;
  L.place = 8 * nw;
  L.cur = 16 * nw;
  L.hist = 24 * nw;
  L.bytes = L.hist + 4 * 256;
  return L;
}

// ------------------------------------------------------------------- prep
#ifndef KAD_PREP_CPL
#define KAD_PREP_CPL 4
#endif
constexpr int PREP_CPL = KAD_PREP_CPL;                 // chunks per lane

// ------------------------------------------------------------- work queue
constexpr int WQ_BATCH = 4;  // units per dequeue

// ------------------------------------------------------------------- lean
constexpr int LEAN_QMAX_DYN = 4;
constexpr int LEAN_BATCH = 4;  // units per work-queue batch (one VGPR of UnitRecs)
static_assert(LEAN_BATCH == WQ_BATCH, "the lean kernel dequeues WQ_BATCH units per ticket");
KAD_HD constexpr int lean_qmax(int nch_t) { return nch_t > 0 ? nch_t : LEAN_QMAX_DYN; }
// cached attributes: alloc/used cpu & mem, NS|NE taints, GVK word 0 (always),
// NE taints (taint filter and some unit has CurrentClusters), PNS taints (TaintToleration score)
struct LeanLayout {
  size_t key, idx, pid, posl, posr, bytes;
};
// per-wave region
KAD_HD inline LeanLayout lean_layout(int C, int qmax) {
 (void)C;
  const size_t P = (size_t)qmax * 64;  // positions held in registers
  LeanLayout L;
  L.key = 0;                     // u32[P] replay keys (total - row minimum)
  L.idx = L.key + 4 * P;         // u16[P] feasible position → cluster id (NCH > 0: P = Cp)
  L.posl = L.idx;                // u16[P + 64] replay scratch (partition stoppers; then ranks): idx is
                                 // dead once the scores have read the cluster ids into registers
  L.pid = L.idx + 2 * P + 128;   // u16[P] replay: original position at each position
  L.posr = L.pid + 2 * P;        // u16[P]
  L.bytes = (L.posr + 2 * P + 15) & ~(size_t)15;
  return L;
}
// block-shared cluster cache (NCH > 0): n_attrs arrays of Cp i64
KAD_HD inline size_t lean_cache_bytes(int C, int n_attrs) { return (size_t)n_attrs * 8 * ((C + 63) & ~63); }

// ------------------------------------------------------------------- wide
constexpr int WIDE_MAX_NCH = 16;
constexpr int WIDE_THREADS = 1024;
#ifndef KAD_WIDE_ZS
#define KAD_WIDE_ZS 1  // the wide kernel's per-cluster zero-request resource scores (c_zs)
#endif
struct WideLayout {
  size_t key, idx, pid, posl, posr, bytes;
};
KAD_HD inline WideLayout wide_layout() {
  WideLayout L;
  L.key = 0;                      // u32[P] replay keys / histogram
  L.idx = L.key + 4 * WIDE_P;     // u16[P] position -> cluster id
  L.posl = L.idx;                 // u16[P + 64] replay scratch, then ranks (idx is dead by then: the
                                  // cluster ids are in registers)
  L.pid = L.idx + 2 * WIDE_P + 128;  // u16[P] replay: original position
  L.posr = L.pid + 2 * WIDE_P;    // u16[P]
  L.bytes = L.posr + 2 * WIDE_P;
  return L;
}
// the compaction stores every feasible cluster's id at its position, even past P (up to 64*nch):
// those land in pid / posr of the same wave's region and the unit is deferred
static_assert(2 * 64 * WIDE_MAX_NCH <= 6 * WIDE_P, "idx overflow past P must stay in the wave's region");
// block-shared cluster cache: av (f64 x2), tg (u64 x2: NS|NE taints, GVK word),
// cap (f64 x2), iv (f32 x2), [ne u64], [pn u64]
KAD_HD inline size_t wide_cache_bytes(int C, int cache_ne, int cache_pn, int cache_zs = 0) {
  const size_t Cp = (size_t)((C + 63) & ~63);
  return Cp * (16 + 16 + 16 + 8 + 8 * cache_ne + 8 * cache_pn + 4 * cache_zs);
}

// -------------------------------------------------------------------- row
constexpr int ROW_THREADS = 512;
constexpr int ROW_WAVES = ROW_THREADS / 64;
constexpr int ROW_MAX_WAVES = 16;  // the row body also runs on schedule_wide_kernel's 1024-thread blocks
constexpr int ROW_MAX_C = 12288;
constexpr int ROW_MAX_BLOCKS = 1024;  // schedule_row_kernel grid cap (its global slabs are sized for it)
constexpr int ROW_NREP = 2048;    // replays of up to this many positions keep their scratch in LDS
constexpr int ROW_BLOCK_PART = 256;  // replay partitions of longer ranges run on every wave of the block
struct RowKLayout {
  size_t key, idx, x, pid, posl, posr, sw, cnt, hist, red, pre, bytes;
};
// a unit's staged record and score program (u32[2][ROW_PRE_DW], the next unit's prefetched into the other
// buffer): its UnitRec dwords, the program length, then its first ROW_PRE_PROG program words
constexpr int ROW_PRE_PROG = 64, ROW_PRE_DW = 16 + 1 + ROW_PRE_PROG + 15;
KAD_HD inline RowKLayout rowk_layout(int C) {
  const size_t Cp = (size_t)((C + 63) & ~63), nch = Cp / 64;
  RowKLayout L;
  L.key = 0;                              // u32[Cp]: fixed | TT raw << 16, then totals (sign-flipped), replay keys
  L.idx = L.key + 4 * Cp;                 // u16[Cp]: position → cluster id
  L.x = L.idx + 2 * Cp;                   // preferred-term words u64[8][nch] while scoring, then the replay
  L.pid = L.x;                            //   scratch: pid u16[NREP], posl u16[NREP + 64], posr u16[NREP]
  L.posl = L.pid + 2 * ROW_NREP;
  L.posr = L.posl + 2 * ROW_NREP + 128;
  const size_t xb = Cp > 6 * (size_t)ROW_NREP + 128 ? Cp : 6 * (size_t)ROW_NREP + 128;
  L.sw = (L.x + xb + 15) & ~(size_t)15;   // u64[2][nch]: the unit's static words (two buffers: the next
  L.cnt = L.sw + 16 * nch;                //   unit's are prefetched); i32[2][nch + 1]: chunk counts →
                                          //   exclusive prefix (+ total)
  L.hist = (L.cnt + 8 * (nch + 1) + 15) & ~(size_t)15;  // u32[256]
  L.red = L.hist + 4 * 256;               // i32[4][ROW_MAX_WAVES] per-wave partials, i32[24] broadcasts
  L.pre = L.red + 4 * (4 * ROW_MAX_WAVES + 24);  // u32[2][ROW_PRE_DW]: staged records + score programs
  L.bytes = L.pre + 4 * 2 * ROW_PRE_DW;
  return L;
}

}  // namespace kad
