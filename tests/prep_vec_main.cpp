// The host's choice between prep_kernel's 8-byte and 16-byte row accesses (csrc/kad_route.h: rows_aligned16,
// prep_vec_ok, route_schedule's r.prep), on the host alone: no HIP header, no device. tests/test_prep_vec_host.py
// compiles this with the host compiler under AddressSanitizer and UndefinedBehaviorSanitizer and runs it.
#include <cstdio>
#include <cstdlib>

#include "../kubeadmiral_amd/csrc/kad_route.h"

using namespace kad;

static int fails = 0;
#define CHECK(x)                                             \
  do {                                                       \
    if (!(x)) {                                              \
      std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #x); \
      fails++;                                               \
    }                                                        \
  } while (0)

static int prep_of(int C, int rows16, int prep_wave = 1) {
  RouteIn in{};
  in.C = C, in.clean = 1, in.fold = 1, in.fitfold = 1, in.TW = 1, in.W = 1000, in.n_cu = 256, in.side_stream = 1;
  in.prep_wave = prep_wave;
  in.rows16 = rows16;
  return route_schedule(in).prep;
}

int main() {
  // addresses: a 64-byte aligned block, and offsets into it (never dereferenced)
  alignas(64) static unsigned char block[256];
  const void* a0 = block;
  const void* a16 = block + 16;
  const void* a32 = block + 32;
  const void* a8 = block + 8;   // 8-byte aligned only: what a uint64_t table is guaranteed
  const void* a24 = block + 24;
  const void* a4 = block + 4;
  CHECK(rows_aligned16({}) == 1);
  CHECK(rows_aligned16({a0}) == 1);
  CHECK(rows_aligned16({a0, a16, a32}) == 1);
  CHECK(rows_aligned16({nullptr, a16, nullptr}) == 1);  // absent tables are never read
  CHECK(rows_aligned16({a8}) == 0);
  CHECK(rows_aligned16({a24}) == 0);
  CHECK(rows_aligned16({a4}) == 0);
  // one 8-byte aligned base among aligned ones, in every position of the seven prep reads or writes
  for (int bad = 0; bad < 7; bad++) {
    const void* p[7] = {a0, a16, a32, a0, a16, a32, a0};
    p[bad] = a8;
    CHECK(rows_aligned16({p[0], p[1], p[2], p[3], p[4], p[5], p[6]}) == 0);
  }

  // prep_vec_ok: whole lanes and aligned bases, both
  for (int nch = 0; nch <= 1024; nch++) {
    CHECK(prep_vec_ok(nch, 1) == (nch > 0 && nch % PREP_CPL == 0));
    CHECK(prep_vec_ok(nch, 0) == false);
  }

  // the route: C by chunk count, with aligned and with unaligned bases
  for (int C = 0; C <= 65535; C++) {
    const int nch = route_nch(C), cw = (nch + 63) / 64;
    const bool wave = nch > 64 && cw <= 4;
    const int want16 = wave ? PREP_WAVE2 + (cw - 2) : (nch > 0 && nch % 4 == 0 ? PREP_VEC : PREP);
    const int want8 = wave ? PREP_WAVE2 + (cw - 2) : PREP;
    if (prep_of(C, 1) != want16 || prep_of(C, 0) != want8) {
      std::printf("FAIL C=%d nch=%d: prep %d / %d, want %d / %d\n", C, nch, prep_of(C, 1), prep_of(C, 0), want16, want8);
      fails++;
      break;
    }
  }
  // the bench shapes and their neighbours, written out
  CHECK(prep_of(1000, 1) == PREP_VEC && prep_of(512, 1) == PREP_VEC && prep_of(256, 1) == PREP_VEC);
  CHECK(prep_of(450, 1) == PREP_VEC && prep_of(705, 1) == PREP_VEC);
  CHECK(prep_of(300, 1) == PREP && prep_of(960, 1) == PREP && prep_of(64, 1) == PREP && prep_of(0, 1) == PREP);
  CHECK(prep_of(1000, 0) == PREP && prep_of(256, 0) == PREP);
  CHECK(prep_of(10000, 1) == PREP_WAVE3 && prep_of(8192, 1) == PREP_WAVE2);
  CHECK(prep_of(8192, 1, 0) == PREP_VEC && prep_of(8192, 0, 0) == PREP);  // 128 chunks without the wave kernel
  CHECK(prep_of(32768, 1) == PREP_VEC && prep_of(32769, 1) == PREP);
  // the lanes per unit are the same on both routes
  {
    RouteIn in{};
    in.C = 1000, in.clean = 1, in.W = 10, in.n_cu = 256;
    const Route r8 = route_schedule(in);
    in.rows16 = 1;
    const Route r16 = route_schedule(in);
    CHECK(r8.prep_lanes == 4 && r16.prep_lanes == 4 && r8.variant == r16.variant && r8.lds == r16.lds);
  }
  if (fails) return 1;
  std::printf("ok: prep route by chunk count and row alignment\n");
  return 0;
}
