// Requirement-row, resource-column and value-row kernels: the snapshot's and the batch's bitmask rows.
// Part of kad_kernels.hip's translation unit, which includes the kernels' headers in definition order.
#pragma once

#include "kad_device.h"
#include "kad_wave.h"

namespace kad {

// ---------------------------------------------------------- predicate programs
// labels.Requirement.Matches / fields one-term selectors (apimachinery v0.26.6) per interned
// requirement and cluster. Requirement × cluster bitmask rows: M[r][ch] bit l = requirement r holds on
// cluster 64*ch + l. Every distinct requirement of the batch is evaluated once per cluster here, instead
// of once per (unit, cluster) pair.
// req_mask_kernel: one wave per (segment of <= 64 requirements on ONE label key, group of REQ_G
// consecutive chunks). The wave loads the key's label-value ids (and, when the segment has Gt/Lt, the
// parsed integers) of its REQ_G chunks once — one coalesced row load per chunk for the whole segment,
// not per requirement — and the segment's requirement words into lanes (lane i = requirement i: op,
// count, first four value ids / the threshold), so the per-requirement loop reads its operands with
// v_readlane: compares, one ballot per chunk, one coalesced store of the REQ_G words (lane j = chunk).
constexpr int REQ_G = REQ_SEG_G;
__global__ __launch_bounds__(256) void req_mask_kernel(SnapDev s, BatchDev b, int ngrp) {
  const int lane = lane_id();
  const int C = s.C, nch = (C + 63) >> 6;
  const long gw = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (gw >= (long)b.n_seg * ngrp) return;
  const int sg = (int)(gw / ngrp), g0 = (int)(gw % ngrp) * REQ_G;
  const int ng = nch - g0 < REQ_G ? nch - g0 : REQ_G;
  const int key = ldc(&b.req_seg[sg].x), first = ldc(&b.req_seg[sg].y), cnt = ldc(&b.req_seg[sg].z);
  // lane i < cnt: requirement i of the segment (id, word offset, op | n << 8, key word, payload 0..3)
  const bool li = lane < cnt;
  const int4* ent = reinterpret_cast<const int4*>(b.req_perm) + 2 * (size_t)(first + (li ? lane : 0));
  const int4 e0 = ent[0], e1 = ent[1];
  const int rid = e0.x, off = e0.y, w0 = li ? e0.z : 0, kw = e0.w;
  const int pv[4] = {e1.x, e1.y, e1.z, e1.w};
  uint64_t* out = b.req_mask;
  // every segment holds requirements on one label key (key >= 0): the label-free ops (TRUE / FALSE /
  // metadata.name =, !=) always take req_row_kernel (kad_batch_upload's routing)
  int32_t lv[REQ_G];
#pragma unroll
  for (int j = 0; j < REQ_G; ++j) {
    const int c = (g0 + j) * WAVE + lane;
    lv[j] = (j < ng && c < C) ? ldg(s.lval, (uint32_t)(key * C + c)) : -1;
  }
  const int op_l = w0 & 0xff;
  const bool has_int = ballot(li && (op_l == KAD_OP_GT || op_l == KAD_OP_LT)) != 0;
  int64_t lint[REQ_G];
  bool lok[REQ_G];
#pragma unroll
  for (int j = 0; j < REQ_G; ++j) {
    lint[j] = 0;
    lok[j] = false;
  }
  if (has_int) {
#pragma unroll
    for (int j = 0; j < REQ_G; ++j) {
      const int c = (g0 + j) * WAVE + lane;
      const uint32_t cc = (j < ng && c < C) ? (uint32_t)(key * C + c) : 0u;
      lint[j] = ldg(s.lint, cc);
      lok[j] = ldg(s.lok, cc) != 0;
    }
  }
  for (int i = 0; i < cnt; ++i) {
    const int wi = __builtin_amdgcn_readlane(w0, i);
    const int op = wi & 0xff, n = (int)((uint32_t)wi >> 8);
    const int r = __builtin_amdgcn_readlane(rid, i);
    bool hit[REQ_G];
    if (op == KAD_OP_GT || op == KAD_OP_LT) {
      const int64_t thr = (int64_t)(((uint64_t)(uint32_t)__builtin_amdgcn_readlane(pv[1], i) << 32) |
                                    (uint32_t)__builtin_amdgcn_readlane(pv[0], i));
#pragma unroll
      for (int j = 0; j < REQ_G; ++j) hit[j] = lv[j] >= 0 && lok[j] && (op == KAD_OP_GT ? lint[j] > thr : lint[j] < thr);
    } else if (op == KAD_OP_EXISTS || op == KAD_OP_DNE) {
#pragma unroll
      for (int j = 0; j < REQ_G; ++j) hit[j] = (lv[j] >= 0) == (op == KAD_OP_EXISTS);
    } else {  // IN / NOTIN / EQ: value ids of this key (>= 0; a missing label is -1)
#pragma unroll
      for (int j = 0; j < REQ_G; ++j) hit[j] = false;
#pragma unroll
      for (int t = 0; t < 4; ++t)
        if (t < n) {
          const int a = __builtin_amdgcn_readlane(pv[t], i);
#pragma unroll
          for (int j = 0; j < REQ_G; ++j) hit[j] |= lv[j] == a;
        }
      if (n > 4) {
        const int offi = __builtin_amdgcn_readlane(off, i);
        for (int t = 4; t < n; ++t) {
          const int a = ldc(b.req + offi + 2 + t);
#pragma unroll
          for (int j = 0; j < REQ_G; ++j) hit[j] |= lv[j] == a;
        }
      }
      if (op == KAD_OP_NOTIN)
#pragma unroll
        for (int j = 0; j < REQ_G; ++j) hit[j] = !hit[j];  // NotIn: a missing label matches too
    }
    uint64_t acc = 0;
#pragma unroll
    for (int j = 0; j < REQ_G; ++j) {
      const int c = (g0 + j) * WAVE + lane;
      const uint64_t m = ballot(hit[j] && c < C && j < ng);
      acc = lane == j ? m : acc;
    }
    if (lane < ng) out[(size_t)r * nch + g0 + lane] = acc;
  }
}

// req_row_kernel: one lane per (value-row requirement, REQ_RC consecutive chunks): In / Equals = OR of the
// value rows, NotIn = its complement (a missing label matches), Exists / DoesNotExist = the key row or its
// complement; TRUE / FALSE / metadata.name =, != are constants or one bit (no loads). The requirement's
// 32-B entry is read once per lane for its REQ_RC words (C5: 100k requirements x 157 chunks).
constexpr int REQ_RC = 4;
__global__ __launch_bounds__(256) void req_row_kernel(SnapDev s, BatchDev b, int zero_rows) {
  const int nch = (s.C + 63) >> 6;
  const int nq = (nch + REQ_RC - 1) / REQ_RC;
  const long g = (long)blockIdx.x * 256 + threadIdx.x;
  // the row list (rows_n, rows_head) emptied before prep_kernel appends to it (early routing): here
  // instead of a separate memset launch
  if (zero_rows && g < 2) b.rows_n[g] = 0;
  if (g >= (long)b.n_rowreq * nq) return;
  const int i = (int)(g / nq), ch0 = (int)(g - (long)i * nq) * REQ_RC;
  const int4 e0 = b.req_rows[2 * (size_t)i], e1 = b.req_rows[2 * (size_t)i + 1];
  const int rid = e0.x, op = e0.y & 0xff, n = (int)((uint32_t)e0.y >> 8), key = e0.z;
  const int v[VR_MAX_VALS] = {e0.w, e1.x, e1.y, e1.z, e1.w};
  const uint64_t tail = (s.C & 63) ? (1ull << (s.C & 63)) - 1 : ~0ull;  // clusters past C: never
  uint64_t* out = b.req_mask + (size_t)rid * nch;
  if (op == KAD_OP_TRUE || op == KAD_OP_FALSE || op == KAD_OP_NAME_EQ || op == KAD_OP_NAME_NE) {
    // label-free: metadata.name = / != the cluster with snapshot id `key` (-1: no such cluster)
#pragma unroll
    for (int k = 0; k < REQ_RC; ++k) {
      const int ch = ch0 + k;
      if (ch >= nch) break;
      const uint64_t one = (key >= 0 && (key >> 6) == ch) ? 1ull << (key & 63) : 0ull;
      uint64_t acc = op == KAD_OP_TRUE ? ~0ull : op == KAD_OP_FALSE ? 0ull : op == KAD_OP_NAME_EQ ? one : ~one;
      if (ch == nch - 1) acc &= tail;
      out[ch] = acc;
    }
    return;
  }
  const uint64_t* kr = s.vrows + (size_t)key * (VR_SLOTS + 1) * nch;
  uint64_t acc[REQ_RC];
#pragma unroll
  for (int k = 0; k < REQ_RC; ++k) acc[k] = 0;
  auto or_row = [&](const uint64_t* row) {  // the lane's REQ_RC words of one value row, loads issued together
    uint64_t w[REQ_RC];
#pragma unroll
    for (int k = 0; k < REQ_RC; ++k) w[k] = ch0 + k < nch ? row[ch0 + k] : 0ull;
#pragma unroll
    for (int k = 0; k < REQ_RC; ++k) acc[k] |= w[k];
  };
  if (op == KAD_OP_EXISTS || op == KAD_OP_DNE) {
    or_row(kr + (size_t)VR_SLOTS * nch);
  } else {
#pragma unroll
    for (int t = 0; t < VR_MAX_VALS; ++t)
      if (t < n) or_row(kr + (size_t)v[t] * nch);
  }
  const bool neg = op == KAD_OP_NOTIN || op == KAD_OP_DNE;
#pragma unroll
  for (int k = 0; k < REQ_RC; ++k) {
    const int ch = ch0 + k;
    if (ch >= nch) break;
    uint64_t x = neg ? ~acc[k] : acc[k];
    if (ch == nch - 1) x &= tail;
    out[ch] = x;
  }
}

// SnapDev::res4 / res_iv (clean snapshots): the same expressions as the wide kernel's block cache
__global__ __launch_bounds__(256) void res_cols_kernel(SnapDev s, double4* r4, float2* iv, ulonglong4* p4) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= s.C) return;
  double capc, avc, capm, avm;
  score_res(s.alloc_cpu[c], s.used_cpu[c], capc, avc);
  score_res(s.alloc_mem[c], s.used_mem[c], capm, avm);
  r4[c] = make_double4(avc, avm, capc, capm);
  iv[c] = make_float2((float)(100.0 / capc), (float)(100.0 / capm));
  if (p4) {
    const int TW = s.TW;
    p4[c] = make_ulonglong4(TW > 0 ? s.pns[c] : 0ull, TW > 1 ? s.pns[(size_t)s.C + c] : 0ull,
                            TW > 2 ? s.pns[2 * (size_t)s.C + c] : 0ull, TW > 3 ? s.pns[3 * (size_t)s.C + c] : 0ull);
  }
}

// SnapDev::vrows: one wave per (key, chunk), lane = cluster; lane s < VR_SLOTS collects value s's word
__global__ __launch_bounds__(256) void value_rows_kernel(SnapDev s, uint64_t* out) {
  const int lane = lane_id();
  const int nch = (s.C + 63) >> 6;
  const long gw = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (gw >= (long)s.K * nch) return;
  const int k = (int)(gw / nch), ch = (int)(gw % nch);
  const int c = ch * WAVE + lane;
  const int v = c < s.C ? ldg(s.lval, (uint32_t)(k * s.C + c)) : -1;
  uint64_t mine = 0;
  for (int t = 0; t < VR_SLOTS; ++t) {
    const uint64_t m = ballot(v == t);
    mine = lane == t ? m : mine;
  }
  const uint64_t has = ballot(v >= 0);
  uint64_t* kr = out + (size_t)k * (VR_SLOTS + 1) * nch + ch;
  kr[(size_t)lane * nch] = mine;
  if (lane == 0) kr[(size_t)VR_SLOTS * nch] = has;
}

}  // namespace kad
