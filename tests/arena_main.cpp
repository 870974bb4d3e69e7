// Stand-alone host check of the staging arena's layout (csrc/kad_arena.h) and the shared CSR validation
// (csrc/kad_ctx.h: first_bad, off_bad, csr_bad). No HIP, no device: tests/test_arena_host.py compiles this with
// the host compiler under -fsanitize=address,undefined and runs it. Prints "ok: N checks" or the first failure.
#define KAD_HOST_ONLY
#include <cstdint>
#include <cstdio>
#include <cstdlib>
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

// parts in declaration order: each on a 256-B boundary, none overlapping the next, the sum = total()
static void check_parts(const Arena& a, const std::vector<Part>& parts, size_t want_total) {
  size_t end = 0;
  for (const Part& p : parts) {
    if (p.at == Arena::ABSENT) continue;
    CHECK(p.at % 256 == 0);
    CHECK(p.at >= end);
    end = p.at + slot(p.bytes);
  }
  CHECK(end <= a.total());
  CHECK(a.total() == want_total);
  CHECK(a.total() % 256 == 0);
}

static void basic() {
  Arena a;
  int x[3] = {1, 2, 3};
  const Part p0 = a.in(x, sizeof x), p1 = a.in(nullptr, 0), p2 = a.in(x, 0), p3 = Arena::absent(), p4 = a.out(257),
             p5 = a.in(x, 4, 4), p6 = a.out(0);
  check_parts(a, {p0, p1, p2, p3, p4, p5, p6}, 256 + 256 + 256 + 512 + 256 + 256);
  CHECK(p0.at == 0 && p1.at == 256 && p2.at == 512 && p4.at == 768 && p5.at == 1280 && p6.at == 1536);
  CHECK(p5.bytes == 4);  // the pad is reserved, not copied
  CHECK(a.inputs().size() == 2);  // only non-empty inputs with a source are copied
  CHECK(a.inputs()[0].h == x && a.inputs()[0].bytes == sizeof x && a.inputs()[1].at == p5.at);
  std::vector<char> buf(a.total());
  CHECK(Arena::ptr<char>(buf.data(), p3) == nullptr);                // absent
  CHECK(Arena::ptr<char>(buf.data(), p1) == buf.data() + 256);       // empty: its own slot
  CHECK(Arena::ptr<char>(buf.data(), p6) == buf.data() + 1536);
  CHECK(Arena::ptr<int>(buf.data(), p0) == reinterpret_cast<int*>(buf.data()));
  Arena e;
  CHECK(e.total() == 0);
}

// The five consumer layouts, declared as their host halves declare them (n scales every count), against the
// closed-form sum of their slots.
static void layouts(size_t n) {
  const char* h = "x";  // any non-null source
  {                     // kad_result_diff: W = n units, n placements, n overrides
    Arena a;
    std::vector<Part> p = {a.in(h, 4 * (n + 1)), a.in(h, 4 * n, 4), a.in(h, 4 * (n + 1)), a.in(h, 4 * n, 4),
                           a.in(h, 8 * n, 8),    a.in(h, n),        a.in(h, n, 1),        a.out(4 * n)};
    check_parts(a, p, 2 * slot(4 * (n + 1)) + 2 * slot(4 * n + 4) + slot(8 * n + 8) + slot(n) + slot(n + 1) + slot(4 * n));
  }
  {  // kad_explain: n units, C = 3, without fit_detail
    Arena a;
    std::vector<Part> p = {a.in(h, 4 * n), a.out(20 * n), a.out(4 * n), Arena::absent(), a.out(n * 3)};
    check_parts(a, p, 2 * slot(4 * n) + slot(20 * n) + slot(3 * n));
  }
  {  // kad_override_match, explicit placements: n objects, n slots, 1 rule word; then from results
    Arena a;
    std::vector<Part> p = {a.in(h, 8 * n), a.in(h, 4 * (n + 1)), a.in(h, 4 * n), a.out(4 * n), a.out(4 * n)};
    check_parts(a, p, slot(8 * n) + slot(4 * (n + 1)) + 3 * slot(4 * n));
    Arena r;
    std::vector<Part> q = {r.in(h, 8 * n), Arena::absent(), Arena::absent(), r.out(4 * n), r.out(4 * n)};
    check_parts(r, q, slot(8 * n) + 2 * slot(4 * n));
  }
  {  // kad_follower_union, explicit leaders without keep: n leaders, n followers, n ids each, capacity n
    Arena a;
    const size_t blocks = (n + 1023) / 1024;
    std::vector<Part> p = {a.in(h, 4 * (n + 1)), a.in(h, 4 * n), Arena::absent(),      a.in(nullptr, 0), Arena::absent(),
                           a.in(nullptr, 0),     a.in(h, 4 * (n + 1)), a.in(h, 4 * n), a.in(h, 4 * (n + 1)),
                           a.in(h, 4 * n),       a.in(h, n),     a.out(n),             a.out(4 * n),     a.out(8 * (n + 1)),
                           a.out(8 * blocks),    a.out(4 * n)};
    check_parts(a, p, 3 * slot(4 * (n + 1)) + 5 * slot(4 * n) + 2 * slot(0) + 2 * slot(n) + slot(8 * (n + 1)) + slot(8 * blocks));
  }
  {  // kad_migrate_estimate: n objects, n segments, n pods, n old entries, no long segment
    Arena a;
    std::vector<Part> p = {a.in(h, 4 * (n + 1)), a.in(h, 8 * n), a.in(h, 4 * n), a.in(h, 4 * n), a.in(h, 8 * n), a.in(h, n),
                           a.in(h, 8 * (n + 1)), a.in(h, 8 * n), a.in(h, n),     a.in(nullptr, 0), a.in(h, 4 * (n + 1)),
                           a.in(h, 4 * n),       a.in(h, 8 * n), a.out(4 * n),   a.out(8 * n),   a.out(8 * n),   a.out(n),
                           a.out(4 * n),         a.out(8 * n),   a.out(n)};
    check_parts(a, p, 2 * slot(4 * (n + 1)) + slot(8 * (n + 1)) + 5 * slot(4 * n) + 7 * slot(8 * n) + 4 * slot(n) + slot(0));
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
  for (size_t n : {(size_t)0, (size_t)1, (size_t)65537}) layouts(n);
  for (int64_t n : {(int64_t)0, (int64_t)1, (int64_t)65537}) csr(n);
  std::printf("ok: %d checks\n", n_checks);
  return 0;
}
