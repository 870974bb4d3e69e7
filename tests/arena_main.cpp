// Stand-alone host check of the staging arena's layout and bound pointers (csrc/kad_arena.h) and the shared CSR validation
// (csrc/kad_ctx.h: first_bad, off_bad, csr_bad). No HIP, no device: tests/test_arena_host.py compiles this with
// the host compiler under -fsanitize=address,undefined and runs it. Prints "ok: N checks" or the first failure.
#define KAD_HOST_ONLY
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../kubeadmiral_amd/csrc/kad_arena.h"
#include "../kubeadmiral_amd/csrc/kad_ctx.h"

static int n_checks = 0;
#define CHECK(x)                                                  \
  do {                                                            \
    n_checks++;                                                   \
    if (!(x)) {                                                   \
      std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #x);  \
      std::exit(1);                                               \
    }                                                             \
  } while (0)

static size_t slot(size_t bytes) { return bytes ? (bytes + 255) / 256 * 256 : 256; }

// parts in declaration order: each on a 256-B boundary, none overlapping the next, the sum = total(); then, placed
// on a dummy base, every bound pointer = base + its part's offset
static void check_parts(const Arena& a, size_t want_parts, size_t want_total) {
  size_t end = 0;
  CHECK(a.parts().size() == want_parts);
  for (const Arena::Part& p : a.parts()) {
    CHECK(p.at % 256 == 0);
    CHECK(p.at >= end);
    end = p.at + slot(p.bytes);
  }
  CHECK(end <= a.total());
  CHECK(a.total() == want_total);
  CHECK(a.total() % 256 == 0);
  char* const base = reinterpret_cast<char*>(uintptr_t(1) << 40);  // never dereferenced
  a.place(base);
  for (const Arena::Part& p : a.parts()) {
    char* got;
    std::memcpy(&got, p.field, sizeof got);
    CHECK(got == base + p.at);
  }
}

static void basic() {
  Arena a;
  int x[3] = {1, 2, 3};
  const int *d0, *d1, *d2, *d3 = x, *d5;
  char *d4, *d6;
  a.in(d0, x, 3);
  a.in(d1, (const int*)nullptr, 0);
  a.in(d2, x, 0);
  a.absent(d3);
  a.out(d4, 257);
  a.in(d5, x, 1, 1);
  a.out(d6, 0);
  check_parts(a, 6, 256 + 256 + 256 + 512 + 256 + 256);
  const std::vector<Arena::Part>& p = a.parts();
  CHECK(p[0].at == 0 && p[1].at == 256 && p[2].at == 512 && p[3].at == 768 && p[4].at == 1280 && p[5].at == 1536);
  CHECK(p[4].bytes == 4);  // the pad is reserved, not copied
  // only non-empty inputs with a source are copied
  CHECK(Arena::copied_in(p[0]) && !Arena::copied_in(p[1]) && !Arena::copied_in(p[2]) && !Arena::copied_in(p[3]) &&
        Arena::copied_in(p[4]) && !Arena::copied_in(p[5]));
  CHECK(p[0].h == x && p[0].bytes == sizeof x && p[4].h == x);
  std::vector<char> buf(a.total());
  a.place(buf.data());
  CHECK(d3 == nullptr);                                        // absent: null, no slot
  CHECK(reinterpret_cast<const char*>(d1) == buf.data() + 256);  // empty: its own slot
  CHECK(d6 == buf.data() + 1536);
  CHECK(d0 == reinterpret_cast<int*>(buf.data()));
  Arena e;
  CHECK(e.total() == 0);
}

// a T of 1, 4 and 8 bytes reserves n * sizeof(T) bytes (+ pad elements), as input and as output
template <class T>
static void widths(size_t n) {
  Arena a;
  std::vector<T> h(n + 1);
  const T* di;
  T *d_out, *d_scratch;
  a.in(di, h.data(), n, 2);
  a.out(d_out, h.data(), n);
  a.out(d_scratch, n);
  for (const Arena::Part& p : a.parts()) CHECK(p.bytes == n * sizeof(T));
  CHECK(a.parts()[1].at == slot(n * sizeof(T) + 2 * sizeof(T)));
  check_parts(a, 3, slot((n + 2) * sizeof(T)) + 2 * slot(n * sizeof(T)));
}

// fetch's list: exactly the non-empty outputs bound to a host destination, in declaration order
static void fetch_list() {
  Arena a;
  int32_t h32[4];
  int64_t h64[4];
  uint8_t h8[4];
  const int32_t* in0;
  int32_t *o0, *o3, *o5 = h32;
  int64_t *o1, *o4;
  uint8_t* o2;
  a.in(in0, h32, 4);
  a.out(o0, h32, 4);
  a.out(o1, 4);                      // device-only
  a.out(o2, h8, 3);
  a.out(o3, (int32_t*)nullptr, 4);   // the caller left the destination out
  a.out(o4, h64, 0);                 // empty
  a.absent(o5);
  a.out(o1, h64, 2);
  std::vector<const Arena::Part*> got;
  for (const Arena::Part& p : a.parts())
    if (Arena::copied_out(p)) got.push_back(&p);
  CHECK(got.size() == 3);
  CHECK(got[0]->back == h32 && got[0]->bytes == 16 && got[0]->field == &o0);
  CHECK(got[1]->back == h8 && got[1]->bytes == 3 && got[1]->field == &o2);
  CHECK(got[2]->back == h64 && got[2]->bytes == 16 && got[2]->field == &o1);
  CHECK(o5 == nullptr);
  for (const Arena::Part& p : a.parts()) CHECK(!(Arena::copied_in(p) && Arena::copied_out(p)));
}

// The consumer layouts, declared as their host halves declare them (n scales every count), against the
// closed-form sum of their slots. One dummy pointer per width stands for every field of that width.
static void layouts(size_t n) {
  static const uint8_t h8[1] = {0};  // any non-null source
  static const int32_t h32[1] = {0};
  static const int64_t h64[1] = {0};
  struct F {  // bound fields: a layout binds each at most once
    const uint8_t* b[24];
    const int32_t* w[24];
    const int64_t* q[24];
    uint8_t* ob[12];
    int32_t* ow[12];
    int64_t* oq[12];
  };
  const int32_t* const no32 = nullptr;
  {  // kad_result_diff: W = n units, n placements, n overrides
    Arena a;
    F f;
    a.in(f.w[0], h32, n + 1), a.in(f.w[1], h32, n, 1), a.in(f.w[2], h32, n + 1), a.in(f.w[3], h32, n, 1);
    a.in(f.q[0], h64, n, 1), a.in(f.b[0], h8, n), a.in(f.b[1], h8, n, 1), a.out(f.ow[0], n);
    check_parts(a, 8, 2 * slot(4 * (n + 1)) + 2 * slot(4 * n + 4) + slot(8 * n + 8) + slot(n) + slot(n + 1) + slot(4 * n));
  }
  {  // kad_explain: n units, C = 3, without fit_detail
    Arena a;
    F f;
    a.in(f.w[0], h32, n), a.out(f.ow[0], 5 * n), a.out(f.ow[1], n), a.absent(f.ow[2]), a.out(f.ob[0], n * 3);
    check_parts(a, 4, 2 * slot(4 * n) + slot(20 * n) + slot(3 * n));
    CHECK(f.ow[2] == nullptr);
  }
  {  // kad_override_match, explicit placements: n objects, n slots, 1 rule word; then from results
    Arena a;
    F f;
    a.in(f.w[0], h32, 2 * n), a.in(f.w[1], h32, n + 1), a.in(f.w[2], h32, n), a.out(f.ow[0], n), a.out(f.ow[1], n);
    check_parts(a, 5, slot(8 * n) + slot(4 * (n + 1)) + 3 * slot(4 * n));
    Arena r;
    r.in(f.w[0], h32, 2 * n), r.absent(f.w[1]), r.absent(f.w[2]), r.out(f.ow[0], n), r.out(f.ow[1], n);
    check_parts(r, 3, slot(8 * n) + 2 * slot(4 * n));
    CHECK(f.w[1] == nullptr && f.w[2] == nullptr);
  }
  {  // kad_follower_union, explicit leaders without keep: n leaders, n followers, n ids each, capacity n
    Arena a;
    F f;
    const size_t blocks = (n + 1023) / 1024;
    a.in(f.w[0], h32, n + 1), a.in(f.w[1], h32, n), a.absent(f.w[2]), a.in(f.w[3], no32, 0), a.absent(f.w[4]);
    a.in(f.w[5], no32, 0), a.in(f.w[6], h32, n + 1), a.in(f.w[7], h32, n), a.in(f.w[8], h32, n + 1);
    a.in(f.w[9], h32, n), a.in(f.b[0], h8, n), a.out(f.ob[0], n), a.out(f.ow[0], n), a.out(f.oq[0], n + 1);
    a.out(f.oq[1], blocks), a.out(f.ow[1], n);
    check_parts(a, 14, 3 * slot(4 * (n + 1)) + 5 * slot(4 * n) + 2 * slot(0) + 2 * slot(n) + slot(8 * (n + 1)) + slot(8 * blocks));
  }
  {  // kad_migrate_estimate: n objects, n segments, n pods, n old entries, no long segment
    Arena a;
    F f;
    a.in(f.w[0], h32, n + 1), a.in(f.q[0], h64, n), a.in(f.w[1], h32, n), a.in(f.w[2], h32, n), a.in(f.q[1], h64, n);
    a.in(f.b[0], h8, n), a.in(f.q[2], h64, n + 1), a.in(f.q[3], h64, n), a.in(f.b[1], h8, n), a.in(f.w[3], no32, 0);
    a.in(f.w[4], h32, n + 1), a.in(f.w[5], h32, n), a.in(f.q[4], h64, n);
    a.out(f.ow[0], n), a.out(f.oq[0], n), a.out(f.oq[1], n), a.out(f.ob[0], n), a.out(f.ow[1], n), a.out(f.oq[2], n);
    a.out(f.ob[1], n);
    check_parts(a, 20, 2 * slot(4 * (n + 1)) + slot(8 * (n + 1)) + 5 * slot(4 * n) + 7 * slot(8 * n) + 4 * slot(n) + slot(0));
  }
  {  // kad_dispatch_plan: n clusters, objects, namespaces, n entries of each list, capacity n
    Arena a;
    F f;
    a.in(f.b[0], h8, n), a.in(f.b[1], h8, n), a.in(f.w[0], h32, n), a.in(f.w[1], h32, n + 1), a.in(f.w[2], h32, n);
    a.in(f.w[3], h32, n + 1), a.in(f.w[4], h32, n), a.in(f.w[5], h32, n + 1), a.in(f.w[6], h32, n), a.in(f.b[2], h8, n);
    a.in(f.q[0], h64, n + 1);
    a.out(f.ow[0], n), a.out(f.ow[1], n), a.out(f.ow[2], n), a.out(f.ob[0], n), a.out(f.ow[3], n), a.out(f.ob[1], n);
    a.out(f.ob[2], n);
    // the parent's list: cf C, of o, ns 4o, po 4(o+1), pc 4np, no 4(n+1), nc 4nn, oo 4(o+1), oc 4nb, ob nb, fo 8(o+1);
    // cnt 4o, ops 4o, sel 4o, res o, cl 4cap, op cap, st cap
    check_parts(a, 18, 6 * slot(n) + 8 * slot(4 * n) + 3 * slot(4 * (n + 1)) + slot(8 * (n + 1)));
  }
  {  // kad_cluster_resources: n clusters, nodes, pods, entries of each; R = 3; no long cluster (one chunk offset)
    Arena a;
    F f;
    a.in(f.q[0], h64, n + 1), a.in(f.b[0], h8, n), a.in(f.q[1], h64, n + 1), a.in(f.b[1], h8, n), a.in(f.q[2], h64, n);
    a.in(f.q[3], h64, n + 1), a.in(f.b[2], h8, n), a.in(f.q[4], h64, n + 1), a.in(f.b[3], h8, n), a.in(f.b[4], h8, n);
    a.in(f.q[5], h64, n), a.in(f.b[5], h8, n), a.in(f.w[0], no32, 0), a.in(f.w[1], h32, 1), a.in(f.w[2], no32, 0);
    a.in(f.q[6], h64, 0), a.in(f.q[7], h64, 0);
    a.out(f.oq[0], 0), a.out(f.oq[1], 3 * n), a.out(f.oq[2], 3 * n), a.out(f.oq[3], n), a.out(f.oq[4], n);
    // the parent's list: cn 8(k+1), nf n, ne 8(n+1), nr en, nv 8en, cp 8(k+1), pf p, pe 8(p+1), pr ep, pk ep, pv 8ep,
    // cl k, ll 4nl, lc 4(nl+1), cc 4nc, lo 8nc, hi 8nc; part 8ncR, alloc 8kR, avail 8kR, has 8k, sn 8k
    check_parts(a, 22, 4 * slot(8 * (n + 1)) + 6 * slot(n) + 4 * slot(8 * n) + 5 * slot(0) + slot(4) + 2 * slot(24 * n));
  }
  {  // kad_status_aggregate, Deployment (NV 5, NOLD 6) then Job (NV 3, NOLD 5): n objects, n segments, none long
    Arena a;
    F f;
    a.in(f.w[0], h32, n + 1), a.in(f.b[0], h8, n), a.in(f.q[0], h64, n), a.in(f.q[1], h64, n), a.in(f.q[2], h64, 6 * n);
    a.in(f.w[1], h32, 5 * n), a.in(f.b[1], h8, n), a.in(f.q[3], h64, n), a.in(f.q[4], h64, n), a.in(f.b[2], h8, n);
    a.in(f.w[2], no32, 0);
    a.out(f.ow[0], 5 * n), a.out(f.ob[0], n), a.out(f.oq[0], n), a.absent(f.oq[1]), a.absent(f.oq[2]), a.absent(f.ow[1]);
    a.absent(f.ow[2]), a.absent(f.ob[1]);
    // the parent's list: so 4(o+1), of o, og 8o, oo 8o, ov 8*6o, sv 4*5s, sf s, sa 8s, sb 8s, ol o, ll 4nl;
    // sums 4*5o, changed o, obs 8o
    check_parts(a, 14, slot(4 * (n + 1)) + 4 * slot(n) + 5 * slot(8 * n) + slot(48 * n) + 2 * slot(20 * n) + slot(0));
    Arena j;
    j.in(f.w[0], h32, n + 1), j.in(f.b[0], h8, n), j.absent(f.q[0]), j.absent(f.q[1]), j.in(f.q[2], h64, 5 * n);
    j.in(f.w[1], h32, 3 * n), j.in(f.b[1], h8, n), j.in(f.q[3], h64, n), j.in(f.q[4], h64, n), j.in(f.b[2], h8, n);
    j.in(f.w[2], no32, 0);
    j.out(f.ow[0], 3 * n), j.out(f.ob[0], n), j.absent(f.oq[0]), j.out(f.oq[1], n), j.out(f.oq[2], n), j.out(f.ow[1], n);
    j.out(f.ow[2], n), j.out(f.ob[1], n);
    // Job: og / oo and obs absent; start 8o, done 8o, nd 4o, nf 4o, fin o
    check_parts(j, 16, slot(4 * (n + 1)) + 5 * slot(n) + 4 * slot(8 * n) + slot(40 * n) + 2 * slot(12 * n) + 2 * slot(4 * n) + slot(0));
  }
  {  // kad_rollout_plan: n objects, n targets (RO_NV = 10 rows of values), none long
    Arena a;
    F f;
    a.in(f.w[0], h32, n + 1), a.in(f.w[1], h32, n), a.in(f.w[2], h32, n), a.in(f.w[3], h32, n), a.in(f.b[0], h8, n);
    a.in(f.w[4], h32, 10 * n), a.in(f.b[1], h8, n), a.in(f.b[2], h8, n), a.in(f.w[5], no32, 0);
    a.out(f.ow[0], n), a.out(f.ow[1], n), a.out(f.ow[2], n), a.out(f.ob[0], n), a.out(f.ob[1], n), a.out(f.ob[2], n);
    // the parent's list: to 4(o+1), ms 4o, mu 4o, rp 4o, of o, tv 4*10t, tf t, om o, ll 4nl; r 4t, s 4t, u 4t, f t, a t, st o
    check_parts(a, 15, slot(4 * (n + 1)) + 6 * slot(4 * n) + 6 * slot(n) + slot(40 * n) + slot(0));
  }
}

// one serial pass: the verdict csr_bad has to give
static bool serial_bad(const int32_t* off, const int32_t* data, int64_t n, int64_t lo, int64_t hi) {
  if (!off || off[0] != 0) return true;
  for (int64_t i = 0; i < n; i++)
    if (off[i + 1] < off[i]) return true;
  if (off[n] && !data) return true;
  for (int64_t j = 0; j < off[n]; j++)
    if (data[j] < lo || data[j] >= hi) return true;
  return false;
}

static void csr(int64_t n) {
  const int64_t lo = -1, hi = 7;
  std::vector<int32_t> off((size_t)n + 1), data((size_t)n, 3);
  for (int64_t i = 0; i <= n; i++) off[(size_t)i] = (int32_t)i;
  auto same = [&](bool want) {
    const bool got = csr_bad(off.data(), data.data(), n, lo, hi);
    CHECK(got == serial_bad(off.data(), data.data(), n, lo, hi));
    CHECK(got == want);
  };
  same(false);
  CHECK(!off_bad(off.data(), n));
  CHECK(csr_bad<int32_t>(nullptr, data.data(), n, lo, hi));
  off[0] = 1;  // a non-zero start
  same(true);
  off[0] = 0;
  if (n == 0) return;
  CHECK(csr_bad(off.data(), nullptr, n, lo, hi));  // data missing when non-empty
  // a decrease at index 0, in the middle, at the last index (and past 65 536 when n reaches there)
  for (int64_t i : {(int64_t)0, n / 2, n - 1, n > 65536 ? (int64_t)65536 : n - 1}) {
    const int32_t keep = off[(size_t)i + 1];
    off[(size_t)i + 1] = off[(size_t)i] - 1;
    CHECK(off_bad(off.data(), n));
    same(true);
    off[(size_t)i + 1] = keep;
  }
  // an entry equal to lo - 1 and to hi, first, in the middle and last; the bounds themselves pass
  for (int64_t j : {(int64_t)0, n / 2, n - 1}) {
    for (int32_t v : {(int32_t)(lo - 1), (int32_t)hi}) {
      data[(size_t)j] = v;
      same(true);
    }
    data[(size_t)j] = (int32_t)lo;
    same(false);
    data[(size_t)j] = (int32_t)(hi - 1);
    same(false);
    data[(size_t)j] = 3;
  }
  // first_bad names the smallest failing index, as a serial pass does
  data[(size_t)(n - 1)] = 99;
  data[(size_t)(n / 2)] = 99;
  CHECK(first_bad(n, [&](int64_t j) { return data[(size_t)j] >= hi; }) == n / 2);
}

int main() {
  basic();
  fetch_list();
  for (size_t n : {(size_t)0, (size_t)1, (size_t)65537}) {
    widths<uint8_t>(n);
    widths<int32_t>(n);
    widths<int64_t>(n);
  }
  for (size_t n : {(size_t)0, (size_t)1, (size_t)65537}) layouts(n);
  for (int64_t n : {(int64_t)0, (int64_t)1, (int64_t)65537}) csr(n);
  std::printf("ok: %d checks\n", n_checks);
  return 0;
}
