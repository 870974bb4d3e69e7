// Override policies (kad_override_match): which override rules match which placed cluster, per object.
//
// The reference asks isClusterMatched (pkg/controllers/override/util.go:154-221) once per (object, placed
// cluster, rule) from parseOverrides (util.go:99-140). A rule's answer depends on the cluster alone, so it is
// computed once per (rule, cluster) into two bitmask rows over the policy set's requirement rows —
// M (matches) and E (isClusterMatched returns an error) — and a batch of objects then only gathers bits:
//
//   override_rule_rows_kernel   one lane per (rule, 64-cluster chunk): the names word, the selector's AND,
//                               the term-by-term walk of MatchClusterSelectorTerms
//                               (util/clusterselector/util.go:97-132) with its error cases kept apart
//   override_status_kernel      one lane per object: does any rule of its first, then of its second policy
//                               have an E bit at a placed cluster (parseOverrides returns on the first error)
//   override_match_kernel       one lane per placed slot: the M bit of every rule of the object's one or two
//                               policies at the slot's cluster, packed into the slot's RW output words
//
// Nothing here writes state that kad_schedule reads.
#include "kad_device.h"
#include "kad_wave.h"

namespace kad {

// M and E of rule r on chunk ch. Lanes of one rule are consecutive chunks, so the requirement-row loads
// are coalesced and the rule's program words (any length: plain loads at pc, no register window) are one
// address per wave, served as a broadcast.
__global__ __launch_bounds__(256) void override_rule_rows_kernel(OverrideDev o) {
  const int nch = (o.C + 63) >> 6;
  const long g = (long)blockIdx.x * 256 + threadIdx.x;
  if (g >= (long)o.R * nch) return;
  const int r = (int)(g / nch), ch = (int)(g - (long)r * nch);
  // clusters past C: never
  const uint64_t all = (ch == nch - 1 && (o.C & 63)) ? (1ull << (o.C & 63)) - 1 : ~0ull;
  const uint32_t f = o.rule_flags[r];
  uint64_t m = 0, e = 0;
  if (!(f & KAD_OVR_HAS_TARGET)) {
    m = all;  // util.go:156-158
  } else {
    // isClusterMatchedByClusterNames (util.go:180-194): the sorted id list's entries inside this chunk
    uint64_t names = all;
    if (f & KAD_OVR_HAS_NAMES) {
      names = 0;
      const int end = o.name_off[r + 1], c0 = ch * WAVE;
      int lo = o.name_off[r], hi = end;
      while (lo < hi) {
        const int mid = lo + ((hi - lo) >> 1);
        if (o.name[mid] < c0)
          lo = mid + 1;
        else
          hi = mid;
      }
      for (int j = lo; j < end; ++j) {
        const int c = o.name[j];
        if (c >= c0 + WAVE) break;
        names |= 1ull << (c - c0);
      }
    }
    if (f & KAD_OVR_SEL_INVALID) {
      e = names;  // util.go:202-207: reached by every cluster that passed the names
    } else {
      const int32_t* P = o.prog + o.prog_off[r];
      const uint64_t* rows = o.req_mask + ch;
      auto row = [&](int id) { return rows[(size_t)id * nch]; };
      int pc = 0;
      const int n_sel = P[pc++];
      uint64_t live = names;
      for (int i = 0; i < n_sel; ++i) live &= row(P[pc++]);
      if (!P[pc++]) {
        m = live;  // util.go:216-218: no ClusterAffinity
      } else {
        // `live`: clusters still walking the terms
        const int n_terms = P[pc++];
        for (int t = 0; t < n_terms && live; ++t) {
          const int tf = P[pc], ne = P[pc + 1], nf = P[pc + 2];
          const int at = pc + 3;
          pc += 3 + ne + nf;
          if (!(tf & (KAD_TERM_HAS_EXPR | KAD_TERM_HAS_FIELD))) continue;  // clusterselector/util.go:103-106
          uint64_t x = live;
          if (tf & KAD_TERM_HAS_EXPR) {
            if (!(tf & KAD_TERM_EXPR_VALID)) {  // :109-112: every cluster that reaches the term
              e |= live;
              break;
            }
            for (int i = 0; i < ne; ++i) x &= row(P[at + i]);
          }
          if (tf & KAD_TERM_HAS_FIELD) {
            if (!(tf & KAD_TERM_FIELD_VALID)) {  // :119-122: only where the expressions matched
              e |= x;
              live &= ~x;
              continue;
            }
            for (int i = 0; i < nf; ++i) x &= row(P[at + ne + i]);
          }
          m |= x;
          live &= ~x;
        }
      }
    }
  }
  if (f & KAD_OVR_BAD_VALUE) e |= m;  // util.go:125-131: unmarshalled only where the rule matched
  o.M[g] = m;
  o.E[g] = e;
}

// the largest i in [0, n) with off[i] <= key (off[0] <= key < off[n])
template <class T>
__device__ __forceinline__ int owner_of(const T* off, int n, int64_t key) {
  int lo = 0, hi = n;  // off[lo] <= key < off[hi]
  while (hi - lo > 1) {
    const int mid = lo + ((hi - lo) >> 1);
    if ((int64_t)off[mid] <= key)
      lo = mid;
    else
      hi = mid;
  }
  return lo;
}

__device__ __forceinline__ bool bit_at(const uint64_t* rows, int nch, int r, int c) {
  return (rows[(size_t)r * nch + (c >> 6)] >> (c & 63)) & 1;
}

__global__ __launch_bounds__(256) void override_status_kernel(OverrideDev o) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= o.n_obj) return;
  const int nch = (o.C + 63) >> 6;
  const int32_t* src = nullptr;
  int n = 0;
  if (!o.from_results) {
    src = o.place_cluster + o.place_off[i];
    n = o.place_off[i + 1] - o.place_off[i];
  } else {
    const int st = o.res_status[i];
    if (st == KAD_ST_OK) {
      src = o.res_cluster + (o.out_off[i] - o.slot_lo);
      n = o.res_count[i];
    } else if (st == KAD_ST_STICKY) {
      src = o.cur_id + o.cur_off[i];
      n = o.cur_off[i + 1] - o.cur_off[i];
    }
  }
  int status = 0;
  for (int q = 0; q < 2 && !status; ++q) {
    const int pol = o.obj_policy[2 * (size_t)i + q];
    if (pol < 0) continue;
    bool err = false;
    for (int r = o.pol_rule_off[pol]; r < o.pol_rule_off[pol + 1]; ++r)
      for (int k = 0; k < n; ++k) {
        const int c = src[k];
        if (c >= 0) err |= bit_at(o.E, nch, r, c);
      }
    if (err) status = q + 1;
  }
  o.status[i] = status;
}

// Slot reads and row writes are one element per lane in lane order (coalesced); the object's policies and
// their rule ranges differ from lane to lane, so they are vector loads (the rule rows they lead to are
// R x nch x 16 B and stay in L2).
__global__ __launch_bounds__(256) void override_match_kernel(OverrideDev o) {
  const int64_t s = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (s >= o.n_slots) return;
  const int nch = (o.C + 63) >> 6;
  int i, c;
  bool placed = true;
  if (!o.from_results) {
    i = owner_of(o.place_off, o.n_obj, s);
    c = o.place_cluster[s];
  } else if (s < o.n_out) {
    const int64_t key = s + o.slot_lo;
    i = owner_of(o.out_off, o.n_obj, key);
    placed = o.res_status[i] == KAD_ST_OK && key - o.out_off[i] < (int64_t)o.res_count[i];
    c = placed ? o.res_cluster[s] : -1;
  } else {
    const int64_t j = s - o.n_out + o.cur_lo;
    i = owner_of(o.cur_off, o.n_obj, j);
    placed = o.res_status[i] == KAD_ST_STICKY;
    c = o.cur_id[j];
  }
  placed = placed && c >= 0 && o.status[i] == 0;
  uint32_t* out = o.matched + (size_t)s * o.RW;
  int j = 0, w = 0;
  uint32_t acc = 0;
  if (placed)
    for (int q = 0; q < 2; ++q) {
      const int pol = o.obj_policy[2 * (size_t)i + q];
      if (pol < 0) continue;
      for (int r = o.pol_rule_off[pol]; r < o.pol_rule_off[pol + 1]; ++r) {  // <= 32 * RW rules (host check)
        acc |= (uint32_t)bit_at(o.M, nch, r, c) << (j & 31);
        if ((++j & 31) == 0) {
          out[w++] = acc;
          acc = 0;
        }
      }
    }
  if (w < o.RW) out[w++] = acc;
  while (w < o.RW) out[w++] = 0;
}

hipError_t launch_override_rule_rows(const OverrideDev& o, hipStream_t st) {
  (void)hipGetLastError();
  const long lanes = (long)o.R * ((o.C + 63) >> 6);
  if (lanes > 0)
    hipLaunchKernelGGL(override_rule_rows_kernel, dim3((unsigned)((lanes + 255) / 256)), dim3(256), 0, st, o);
  return hipGetLastError();
}

hipError_t launch_override_match(const OverrideDev& o, hipStream_t st) {
  (void)hipGetLastError();
  if (o.n_obj > 0)
    hipLaunchKernelGGL(override_status_kernel, dim3((unsigned)((o.n_obj + 255) / 256)), dim3(256), 0, st, o);
  if (o.n_slots > 0)
    hipLaunchKernelGGL(override_match_kernel, dim3((unsigned)((o.n_slots + 255) / 256)), dim3(256), 0, st, o);
  return hipGetLastError();
}

}  // namespace kad

// ------------------------------------------------------ host half: kad_override_*
#include "kad_arena.h"

using namespace kad;

// ------------------------------------------------------ override policies
// A policy-set blob may come from any packer: before it is copied to the device every array is checked to
// lie in the blob, every CSR offset array to be monotone, every id the kernels index with to be in range
// and every target program to be well formed. Host only: sh is the header of the snapshot it was packed for.
static int validate_policies(const void* blob, size_t nbytes, const kad_snapshot_header& sh, kad_override_header* hdr,
                             std::string* err) {
  auto bad = [&](const std::string& m) {
    *err = m;
    return KAD_EINVAL;
  };
  kad_override_header h;
  if (!blob || nbytes < sizeof(h)) return bad("policy set too small");
  std::memcpy(&h, blob, sizeof(h));
  if (h.magic != KAD_OVERRIDE_MAGIC) return bad("bad policy set magic");
  if (h.abi_version != KAD_ABI_VERSION) return bad("policy set ABI version mismatch");
  if (h.total_bytes != nbytes) return bad("policy set size mismatch");
  if (h.snapshot_fingerprint != sh.fingerprint || h.n_clusters != sh.n_clusters)
    return bad("policy set was packed against a different snapshot");
  const int P = h.n_policies, R = h.n_rules, NR = h.n_reqs, C = sh.n_clusters, K = sh.n_label_keys;
  if (P < 0 || R < 0 || NR < 0) return bad("bad policy set counts");
  const char* base = static_cast<const char*>(blob);
  auto extent = [&](int a, uint64_t count) {
    const uint64_t o = h.off[a];
    return o <= nbytes && !(o & 7) && count <= (nbytes - o) / 4;
  };
  auto arr = [&](int a) { return reinterpret_cast<const int32_t*>(base + h.off[a]); };
  // offsets off_a[0 .. n]: from 0, non-decreasing; the data array holds off[n] words
  auto csr = [&](int off_a, int n, int data_a) {
    if (!extent(off_a, (uint64_t)n + 1)) return false;
    const int32_t* o = arr(off_a);
    if (o[0] != 0) return false;
    for (int i = 0; i < n; i++)
      if (o[i + 1] < o[i]) return false;
    return data_a < 0 || extent(data_a, (uint64_t)o[n]);
  };
  if (!csr(KAD_O_POL_RULE_OFF, P, -1) || arr(KAD_O_POL_RULE_OFF)[P] != R)
    return bad("policy rule offsets must run from 0 to n_rules");
  if (!extent(KAD_O_RULE_FLAGS, (uint64_t)R)) return bad("policy set array rule_flags lies outside the blob");
  if (!csr(KAD_O_RULE_NAME_OFF, R, KAD_O_RULE_NAME)) return bad("bad rule name offsets");
  if (!csr(KAD_O_RULE_PROG_OFF, R, KAD_O_RULE_PROG)) return bad("bad rule program offsets");
  if (!csr(KAD_O_REQ_OFF, NR, KAD_O_REQ)) return bad("bad requirement offsets");
  const uint32_t* fl = reinterpret_cast<const uint32_t*>(arr(KAD_O_RULE_FLAGS));
  const int32_t *no = arr(KAD_O_RULE_NAME_OFF), *nm = arr(KAD_O_RULE_NAME);
  const int32_t *po = arr(KAD_O_RULE_PROG_OFF), *pg = arr(KAD_O_RULE_PROG);
  const int32_t *ro = arr(KAD_O_REQ_OFF), *rq = arr(KAD_O_REQ);
  for (int r = 0; r < NR; r++) {  // [op | n << 8, key, payload...], as validate_batch
    const int len = ro[r + 1] - ro[r];
    if (len < 2) return bad("requirement shorter than two words");
    const int32_t* p = rq + ro[r];
    const int op = p[0] & 0xff, n = (int)((uint32_t)p[0] >> 8), key = p[1];
    if (len != 2 + n) return bad("requirement payload length mismatch");
    const bool label_key = key >= 0 && key < K;
    bool ok;
    switch (op) {
      case KAD_OP_IN: case KAD_OP_NOTIN: case KAD_OP_EQ: ok = label_key && n >= 1; break;
      case KAD_OP_EXISTS: case KAD_OP_DNE: ok = label_key && n == 0; break;
      case KAD_OP_GT: case KAD_OP_LT: ok = label_key && n == 2; break;
      case KAD_OP_NAME_EQ: case KAD_OP_NAME_NE: ok = key >= -1 && key < C; break;
      case KAD_OP_TRUE: case KAD_OP_FALSE: ok = true; break;
      default: ok = false;
    }
    if (!ok) return bad("bad requirement " + std::to_string(r));
  }
  for (int r = 0; r < R; r++) {
    if (fl[r] & ~(KAD_OVR_HAS_TARGET | KAD_OVR_HAS_NAMES | KAD_OVR_SEL_INVALID | KAD_OVR_BAD_VALUE))
      return bad("unknown flags of rule " + std::to_string(r));
    for (int j = no[r]; j < no[r + 1]; j++)
      if (nm[j] < 0 || nm[j] >= C || (j > no[r] && nm[j] <= nm[j - 1]))
        return bad("cluster ids of rule " + std::to_string(r) + " must be ascending snapshot ids");
    // the program: every requirement id in range, the structure consumes exactly the rule's words
    const int32_t* p = pg + po[r];
    const int64_t len = po[r + 1] - po[r];
    auto ids_ok = [&](int64_t at, int64_t n) {
      if (n < 0 || at + n > len) return false;
      for (int64_t i = 0; i < n; i++)
        if (p[at + i] < 0 || p[at + i] >= NR) return false;
      return true;
    };
    bool ok = len >= 2;
    int64_t pc = 0;
    if (ok) {
      const int64_t n_sel = p[pc++];
      ok = ids_ok(pc, n_sel);
      pc += ok ? n_sel : 0;
      ok = ok && pc < len;
      if (ok && p[pc++]) {
        ok = pc < len;
        const int64_t n_terms = ok ? p[pc++] : 0;
        ok = ok && n_terms >= 0;
        for (int64_t t = 0; ok && t < n_terms; t++) {
          ok = pc + 3 <= len;
          if (!ok) break;
          const int64_t ne = p[pc + 1], nf = p[pc + 2];
          ok = ne >= 0 && nf >= 0 && ids_ok(pc + 3, ne + nf);
          pc += 3 + (ok ? ne + nf : 0);
        }
      }
    }
    if (!ok || pc != len) return bad("malformed target program of rule " + std::to_string(r));
  }
  *hdr = h;
  return KAD_OK;
}

static int override_policies_upload_locked(kad_ctx* c, const void* blob, size_t nbytes) {
  c->have_ovr = false;  // a failed upload leaves no policy set resident
  if (!c->have_snapshot) return fail(c, KAD_ESTATE, "no snapshot uploaded");
  kad_override_header h;
  std::string err;
  if (int r = validate_policies(blob, nbytes, c->snap_hdr, &h, &err)) return fail(c, r, err);
  HIPCHK(c, hipSetDevice(c->device));
  if (int r = grow(c, c->d_ovr, nbytes)) return r;
  HIPCHK(c, hipMemcpyAsync(c->d_ovr.p, blob, nbytes, hipMemcpyHostToDevice, c->stream));
  const int32_t* pro = at<int32_t>(blob, h.off, KAD_O_POL_RULE_OFF);
  c->h_ovr_pro.assign(pro, pro + h.n_policies + 1);
  const size_t nch = (size_t)((c->sd.C + 63) / 64);
  const ReqRouting rr = route_requirements(h.n_reqs, at<int32_t>(blob, h.off, KAD_O_REQ_OFF),
                                           at<int32_t>(blob, h.off, KAD_O_REQ), c->snap_hdr.n_label_keys, nch,
                                           c->sd.vrows != nullptr, c->h_ovr_reqseg);
  c->ovr_n_seg = rr.n_seg;
  c->ovr_n_rowreq = rr.n_rowreq;
  c->ovr_n_seg_reqs = rr.n_seg_reqs;
  if (int r = grow(c, c->d_ovr_reqseg, c->h_ovr_reqseg.size() * 4 + 16)) return r;
  if (!c->h_ovr_reqseg.empty())
    HIPCHK(c, hipMemcpyAsync(c->d_ovr_reqseg.p, c->h_ovr_reqseg.data(), c->h_ovr_reqseg.size() * 4, hipMemcpyHostToDevice,
                             c->stream));
  if (int r = grow(c, c->d_ovr_rows, ((size_t)h.n_reqs + 2 * (size_t)h.n_rules) * nch * 8)) return r;
  HIPCHK(c, hipStreamSynchronize(c->stream));
  c->ovr_hdr = h;
  c->have_ovr = true;
  return KAD_OK;
}

static int override_match_locked(kad_ctx* c, const kad_override_batch* b, const kad_override_view* out) {
  if (!c->have_snapshot || !c->have_ovr) return fail(c, KAD_ESTATE, "snapshot and policy set must be uploaded first");
  const bool from_results = b->place_off == nullptr;
  if (from_results && (!c->have_batch || !c->ran)) return fail(c, KAD_ESTATE, "nothing has been scheduled");
  const kad_override_header& h = c->ovr_hdr;
  const int n = b->n_objects, RW = b->rule_words, P = h.n_policies, C = c->sd.C;
  if (n < 0 || RW < 1 || (n && (!b->obj_policy || !out || !out->status)))
    return fail(c, KAD_EINVAL, "object list or output view missing");
  if (from_results && n != c->bd.W) return fail(c, KAD_EINVAL, "n_objects differs from the resident batch's units");
  if (!from_results && (b->place_off[0] != 0 || (b->place_off[n] && !b->place_cluster)))
    return fail(c, KAD_EINVAL, "place_off must start at 0");
  const int32_t* pro = c->h_ovr_pro.data();
  {
    const int32_t* op = b->obj_policy;
    const int64_t i = first_bad(n, [&](int64_t i) {
      int64_t rules = 0;
      for (int q = 0; q < 2; q++) {
        const int p = op[2 * i + q];
        if (p < -1 || p >= P) return true;
        if (p >= 0) rules += pro[p + 1] - pro[p];
      }
      return rules > 32 * (int64_t)RW;
    });
    if (i >= 0)
      return fail(c, KAD_EINVAL, "object " + std::to_string(i) + ": policy index out of range, or more than 32 * rule_words rules");
  }
  int64_t n_slots;
  if (from_results) {
    n_slots = c->slot_n + c->cur_n;
  } else {
    // (its start and a missing place_cluster were told apart above, so each check has one message)
    if (off_bad(b->place_off, n)) return fail(c, KAD_EINVAL, "place_off must be non-decreasing");
    n_slots = b->place_off[n];
    if (csr_bad(b->place_off, b->place_cluster, n, -1, C)) return fail(c, KAD_EINVAL, "placed cluster id out of range");
  }
  if (n == 0) return KAD_OK;
  if (n_slots && !out->matched) return fail(c, KAD_EINVAL, "output view missing");
  HIPCHK(c, hipSetDevice(c->device));
  // one buffer: obj_policy, place_off, place_cluster, then status and the matched rows
  OverrideDev o{};
  Arena a;
  a.in(o.obj_policy, b->obj_policy, 2 * (size_t)n);
  if (from_results) {
    a.absent(o.place_off);
    a.absent(o.place_cluster);
  } else {
    a.in(o.place_off, b->place_off, (size_t)n + 1);
    a.in(o.place_cluster, b->place_cluster, (size_t)n_slots);
  }
  a.out(o.status, out->status, (size_t)n);
  a.out(o.matched, out->matched, (size_t)n_slots * RW);
  Stage& stg = c->stage[STG_OVERRIDE];
  if (int r = a.commit(c, stg.buf)) return r;
  const size_t nch = (size_t)((C + 63) / 64);
  const char* base = c->d_ovr.as<const char>();
  uint64_t* rows = c->d_ovr_rows.as<uint64_t>();
  // requirement rows of the set's table: req_row_kernel and req_mask_kernel read these fields only
  BatchDev rb{};
  rb.NR = h.n_reqs;
  rb.req_off = at<int32_t>(base, h.off, KAD_O_REQ_OFF);
  rb.req = at<int32_t>(base, h.off, KAD_O_REQ);
  rb.req_mask = rows;
  rb.n_seg = c->ovr_n_seg;
  rb.req_perm = c->d_ovr_reqseg.as<const int32_t>();
  rb.req_seg = reinterpret_cast<const int4*>(rb.req_perm + (size_t)c->ovr_n_seg_reqs * 8);
  rb.n_rowreq = c->ovr_n_rowreq;
  rb.req_rows = reinterpret_cast<const int4*>(reinterpret_cast<const int32_t*>(rb.req_seg) + 4 * (size_t)c->ovr_n_seg);
  o.C = C;
  o.P = P;
  o.R = h.n_rules;
  o.pol_rule_off = at<int32_t>(base, h.off, KAD_O_POL_RULE_OFF);
  o.rule_flags = at<uint32_t>(base, h.off, KAD_O_RULE_FLAGS);
  o.name_off = at<int32_t>(base, h.off, KAD_O_RULE_NAME_OFF);
  o.name = at<int32_t>(base, h.off, KAD_O_RULE_NAME);
  o.prog_off = at<int32_t>(base, h.off, KAD_O_RULE_PROG_OFF);
  o.prog = at<int32_t>(base, h.off, KAD_O_RULE_PROG);
  o.req_mask = rows;
  o.M = rows + (size_t)h.n_reqs * nch;
  o.E = o.M + (size_t)h.n_rules * nch;
  o.n_obj = n;
  o.RW = RW;
  o.from_results = from_results ? 1 : 0;
  if (from_results) {
    o.out_off = c->bd.out_off;
    o.cur_off = c->bd.cur_off;
    o.cur_id = c->bd.cur_id;
    o.res_status = c->d_status;
    o.res_count = c->d_count;
    o.res_cluster = c->d_cluster;
    o.slot_lo = c->slot_lo;
    o.n_out = c->slot_n;
    o.cur_lo = c->cur_lo;
  }
  o.n_slots = n_slots;
  HIPCHK(c, hipEventRecord(stg.ev[0], c->stream));
  bool zeroed = false;
  HIPCHK(c, launch_req_masks(c->sd, rb, c->stream, false, &zeroed));
  HIPCHK(c, hipEventRecord(stg.ev[1], c->stream));
  HIPCHK(c, launch_override_rule_rows(o, c->stream));
  HIPCHK(c, hipEventRecord(stg.ev[2], c->stream));
  HIPCHK(c, launch_override_match(o, c->stream));
  HIPCHK(c, hipEventRecord(stg.ev[3], c->stream));
  stg.ran = true;
  if (int r = a.fetch(c)) return r;
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return KAD_OK;
}

extern "C" {

// Host only (tests, packers): validate_policies against the header of a packed snapshot blob.
int kad_override_policies_check(const void* blob, size_t nbytes, const void* snapshot_blob, size_t snapshot_nbytes) {
  try {
    kad_snapshot_header sh;
    if (!snapshot_blob || snapshot_nbytes < sizeof(sh)) return KAD_EINVAL;
    std::memcpy(&sh, snapshot_blob, sizeof(sh));
    if (sh.magic != KAD_SNAPSHOT_MAGIC) return KAD_EINVAL;
    kad_override_header h;
    std::string err;
    return validate_policies(blob, nbytes, sh, &h, &err);
  } catch (...) {
    return KAD_EHOST;
  }
}

int kad_override_policies_upload(kad_ctx* c, const void* blob, size_t nbytes) {
  return entry(c, blob != nullptr, [&]() -> int {
    return override_policies_upload_locked(c, blob, nbytes);
  });
}

int kad_override_match(kad_ctx* c, const kad_override_batch* b, const kad_override_view* out) {
  return entry(c, b != nullptr, [&]() -> int {
    return override_match_locked(c, b, out);
  });
}

int kad_override_timing(kad_ctx* c, float ms[3]) { return stage_timing(c, STG_OVERRIDE, 3, ms, "no kad_override_match ran"); }

}  // extern "C"
