// The host functions of csrc/kad_history.h (KAD_HOST_ONLY: no HIP header, no device) in a program of their own, which
// tests/test_history_host.py compiles with the host compiler under AddressSanitizer and UndefinedBehaviorSanitizer:
// the update revision's label parse against snprintf + the alphabet + strtoll, the probe's digits against snprintf, the
// equal-test order, the revision number's wrap, the truncation count at its edges, the kept revision's action, the
// sort key, and the route at O = 0.
#define KAD_HOST_ONLY
#include "../kubeadmiral_amd/csrc/kad_history.h"

#include <cerrno>
#include <climits>
#include <cstdio>
#include <cstdlib>
#include <cstring>

using namespace kad;

static int fails = 0;
#define CHECK(x)                                              \
  do {                                                        \
    if (!(x)) {                                               \
      std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #x); \
      ++fails;                                                \
    }                                                         \
  } while (0)

static void label_by_string(uint32_t sum, bool* parsed, uint32_t* val) {
  static const char alphabet[] = "bcdfghjklmnpqrstvwxz2456789";
  char dec[16], lab[16];
  std::snprintf(dec, sizeof dec, "%u", sum);
  size_t n = std::strlen(dec);
  for (size_t i = 0; i < n; ++i) lab[i] = alphabet[(unsigned char)dec[i] % 27];
  lab[n] = 0;
  *parsed = false;
  *val = 0;
  for (size_t i = 0; i < n; ++i)
    if (lab[i] < '0' || lab[i] > '9') return;
  errno = 0;
  const long long v = std::strtoll(lab, nullptr, 10);
  if (errno || v > INT32_MAX) return;
  *parsed = true;
  *val = (uint32_t)v;
}

int main() {
  uint32_t x = 12345;
  int n_parsed = 0;
  for (int i = 0; i < 2000000; ++i) {
    x = x * 1664525u + 1013904223u;
    uint32_t s = x;
    if (i % 3 == 0) {  // sums whose digits are all small, of every length
      char buf[16];
      int len = 1 + (int)((x >> 8) % 10);
      for (int k = 0; k < len; ++k) buf[k] = (char)('0' + ((x >> (k * 3)) % 6));
      if (buf[0] == '0') buf[0] = '1';
      buf[len] = 0;
      const unsigned long long v = std::strtoull(buf, nullptr, 10);
      if (v > UINT32_MAX) continue;
      s = (uint32_t)v;
    }
    bool p;
    uint32_t v, w;
    label_by_string(s, &p, &v);
    const bool q = hr_update_label(s, &w);
    CHECK(p == q && v == w);
    n_parsed += q;
  }
  CHECK(n_parsed > 1000);
  const uint32_t edge[] = {0u, 5u, 6u, 9u, 1743039203u, 1743039204u, 555555555u, 1555555555u, 4294967295u};
  for (uint32_t s : edge) {
    bool p;
    uint32_t v, w;
    label_by_string(s, &p, &v);
    CHECK(hr_update_label(s, &w) == p && v == w);
  }
  const int32_t probes[] = {0, 1, 9, 10, -1, -12, 2147483647, INT32_MIN, 1000000000, -1000000000, 99, 100};
  for (int32_t v : probes) {
    char buf[16];
    std::snprintf(buf, sizeof buf, "%d", v);
    CHECK(hr_fnv_i32(2166136261u, v) == hr_fnv_bytes(2166136261u, reinterpret_cast<const uint8_t*>(buf), (int64_t)std::strlen(buf)));
  }
  CHECK(hr_fnv_bytes(2166136261u, reinterpret_cast<const uint8_t*>("a"), 1) == 0x050c5d7eu);
  CHECK(hr_fnv_bytes(2166136261u, reinterpret_cast<const uint8_t*>("foobar"), 6) == 0x31f0b262u);
  // the order of the equal test: length first, then the labels only if both parsed
  CHECK(hr_equal_pre(3, 4, true, 1, true, 1) == 0);
  CHECK(hr_equal_pre(3, 3, true, 1, true, 2) == 0);
  CHECK(hr_equal_pre(3, 3, true, 1, true, 1) == 1);
  CHECK(hr_equal_pre(3, 3, false, 1, true, 2) == 1 && hr_equal_pre(3, 3, true, 1, false, 2) == 1 && hr_equal_pre(0, 0, false, 0, false, 0) == 1);
  CHECK(hr_revision_number(0) == 1 && hr_revision_number(-7) == 1 && hr_revision_number(41) == 42 && hr_revision_number(INT64_MAX) == INT64_MIN);
  CHECK(hr_kill(5, 2) == 3 && hr_kill(5, 5) == 0 && hr_kill(5, 9) == 0 && hr_kill(5, -1) == 5 && hr_kill(0, -1) == 0);
  CHECK(hr_kill(5, INT64_MIN) == 0 && hr_kill(5, INT64_MAX) == 0 && hr_kill(4096, 1) == 4095 && hr_kill(3, INT64_MIN + 1) == 0);
  CHECK(hr_keep_action(1, 2, true) == HR_ACT_RENUMBER && hr_keep_action(2, 2, true) == 0 && hr_keep_action(2, 2, false) == HR_ACT_RELABEL);
  CHECK(hr_keep_action(7, INT64_MIN, false) == HR_ACT_RELABEL);
  CHECK(hr_key_less(1, 9, 9, 9, 2, 0, 0, 0) && !hr_key_less(2, 0, 0, 0, 1, 9, 9, 9));
  CHECK(hr_key_less(1, 1, 9, 9, 1, 2, 0, 0) && hr_key_less(1, 1, 1, 9, 1, 1, 2, 0) && hr_key_less(1, 1, 1, 1, 1, 1, 1, 2));
  CHECK(!hr_key_less(1, 1, 1, 1, 1, 1, 1, 1));
  CHECK(hr_action_cap(0) == 1 && hr_action_cap(4096) == 8193);
  const RevisionRoute r0 = route_revision(0, 0, 0, 0, 0, 0, 256);
  CHECK(r0.grid == 0 && r0.cmp_grid == 0 && r0.hash_grid == 0 && r0.long_grid == 0 && r0.width == 1 && r0.cmp_width == 1);
  const RevisionRoute r1 = route_revision(1000, 900, 2, 998 * 5, 998 * 5 + 600, 200000, 256);
  CHECK(r1.width == 8 && r1.long_grid == 2 && r1.hash_grid == 4 && r1.cmp_width == 16);
  if (fails) return 1;
  std::printf("ok: %d labels parsed\n", n_parsed);
  return 0;
}
