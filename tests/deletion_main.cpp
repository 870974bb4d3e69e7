// kad_deletion_check / kad_deletion_finish_check, kad_deletion_decide and the calls' arena layout in a program of their
// own, which tests/test_deletion_host.py builds together with csrc/kad_deletion.hip (host code under AddressSanitizer
// and UndefinedBehaviorSanitizer, device code as it is) and runs as its own process: a good batch, every array exactly
// as long as the counts say (so that a read past an end is seen), then one malformed batch per rule. No device is
// touched: the checks are host only.
#include "../kubeadmiral_amd/csrc/kad_deletion.h"

#include <cstdio>
#include <vector>

#define KAD_HOST_ONLY
#include "../kubeadmiral_amd/csrc/kad_arena.h"
#undef KAD_HOST_ONLY
#include "../include/kad_sched.h"

namespace kad {
int n_cus() { return 256; }  // (kad_api.hip's, which this program does not link)
}  // namespace kad

using namespace kad;

static int fails = 0;
#define CHECK(x)                                              \
  do {                                                        \
    if (!(x)) {                                               \
      std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #x); \
      ++fails;                                                \
    }                                                         \
  } while (0)

struct Case {
  std::vector<uint8_t> cf, of, obf, ok, wait, kf, ccf;
  std::vector<int32_t> oo, oc, ko, kc;
  std::vector<uint8_t> out_op, pre, first, status, reason, then;
  std::vector<int32_t> n_ops, n_rem, n_rf, n_fo, n_fc;
  kad_deletion_batch b{};
  kad_deletion_view v{};
  kad_deletion_results r{};
  kad_deletion_finish_view fv{};
  void bind() {
    const size_t O = of.size(), B = obf.size();
    out_op.assign(B, 0);
    for (auto* x : {&pre, &first, &status, &reason, &then}) x->assign(O, 0);
    for (auto* x : {&n_ops, &n_rem, &n_rf, &n_fo, &n_fc}) x->assign(O, 0);
    b = kad_deletion_batch{(int32_t)cf.size(), (int32_t)O, cf.data(), of.data(), oo.data(), oc.data(), obf.data()};
    v = kad_deletion_view{out_op.data(), n_ops.data(), n_rem.data(), n_rf.data(), pre.data(), first.data()};
    r = kad_deletion_results{ok.data(), wait.data(), ko.data(), kc.data(), kf.data(), ccf.data()};
    fv = kad_deletion_finish_view{status.data(), reason.data(), then.data(), n_fo.data(), n_fc.data()};
  }
  int plan() { return kad_deletion_check(&b, &v); }
  int finish() { return kad_deletion_finish_check(&b, &fv, &r); }
};

// n objects over C clusters, object i observed in i % 5 clusters from i on (ascending, wrapping avoided)
static Case good(int C, int n) {
  Case c;
  c.cf.assign((size_t)C, 1);
  c.ccf.assign((size_t)C, 9);
  c.oo.push_back(0);
  c.ko.push_back(0);
  for (int i = 0; i < n; ++i) {
    const uint8_t flags[] = {1, 3, 5, 8, 0, 2};
    c.of.push_back(flags[i % 6]);
    c.wait.push_back((uint8_t)(i % 4));
    const int m = i % 5 < C ? i % 5 : C, at = i % (C - m + 1);
    for (int k = 0; k < m; ++k) {
      c.oc.push_back(at + k);
      const uint8_t ob[] = {1, 3, 5, 7, 8};
      c.obf.push_back(ob[(i + k) % 5]);
      c.ok.push_back((uint8_t)((i + k) % 7 != 0));
    }
    c.oo.push_back((int32_t)c.oc.size());
    if (i % 3 == 0 && C > 1) {
      c.kc.push_back(i % C);
      c.kf.push_back((uint8_t)(1u << (i % 4)));
    }
    c.ko.push_back((int32_t)c.kc.size());
  }
  c.bind();
  return c;
}

int main() {
  // ---- the decision, every input
  for (uint32_t of = 0; of < 16; ++of)
    for (int ready = 0; ready < 2; ++ready)
      for (uint32_t ob = 0; ob < 16; ++ob) {
        uint8_t out[3] = {9, 9, 9};
        CHECK(kad_deletion_decide(of, ready, ob, out) == KAD_OK);
        const bool walks = (of & 9) != 0, ex = (ob & 1) && !(ob & 8);
        if (!walks || !ready) CHECK(out[0] == 0 && out[1] == 0 && out[2] == 0);
        if (walks && ready && (ob & 8)) CHECK(out[0] == 0 && out[1] == 0 && out[2] == 1);
        if (walks && ready && ex && !(of & 10)) CHECK(out[1] == 1 && out[0] == (((of & 4) && (ob & 4)) ? 4 : 3));
        if (walks && ready && ex && (of & 10)) CHECK(out[1] == 0 && out[0] == ((ob & 2) ? 0 : 4));
      }
  uint8_t o3[3];
  CHECK(kad_deletion_decide(16, 1, 1, o3) == KAD_EINVAL && kad_deletion_decide(1, 1, 16, o3) == KAD_EINVAL);
  CHECK(kad_deletion_decide(1, 1, 1, nullptr) == KAD_EINVAL);

  // ---- good batches at the sizes around first_bad's parallel threshold
  for (int n : {0, 1, 7, 65535, 65536, 65537}) {
    Case c = good(1000, n);
    CHECK(c.plan() == KAD_OK);
    CHECK(c.finish() == KAD_OK);
  }
  {
    Case c = good(1, 5);
    CHECK(c.plan() == KAD_OK && c.finish() == KAD_OK);
    Case z = good(16384, 3);
    CHECK(z.plan() == KAD_OK && z.finish() == KAD_OK);
  }
  // ---- one malformed batch per rule
  auto bad_plan = [&](const char* what, auto edit, int want = KAD_EINVAL) {
    Case c = good(40, 30);
    edit(c);
    const int got = c.plan();
    if (got != want) {
      std::printf("FAIL plan %s: %d\n", what, got);
      ++fails;
    }
    const int fin = c.finish();
    if (fin != want) {
      std::printf("FAIL finish (plan rule) %s: %d\n", what, fin);
      ++fails;
    }
  };
  auto bad_finish = [&](const char* what, auto edit) {
    Case c = good(40, 30);
    edit(c);
    CHECK(c.plan() == KAD_OK);
    const int got = c.finish();
    if (got != KAD_EINVAL) {
      std::printf("FAIL finish %s: %d\n", what, got);
      ++fails;
    }
  };
  bad_plan("negative clusters", [](Case& c) { c.b.n_clusters = -1; });
  bad_plan("negative objects", [](Case& c) { c.b.n_objects = -1; });
  bad_plan("too many clusters", [](Case& c) { c.b.n_clusters = 16385; }, KAD_EUNSUPPORTED);
  bad_plan("cluster_flags missing", [](Case& c) { c.b.cluster_flags = nullptr; });
  bad_plan("cluster flag unknown", [](Case& c) { c.cf[39] = 16; });
  bad_plan("obj_flags missing", [](Case& c) { c.b.obj_flags = nullptr; });
  bad_plan("object flag unknown", [](Case& c) { c.of[29] = 16; });
  bad_plan("orphan all and adopted", [](Case& c) { c.of[3] = 1 | 2 | 4; });
  bad_plan("possible orphan with finalizer", [](Case& c) { c.of[3] = 8 | 1; });
  bad_plan("possible orphan with orphan", [](Case& c) { c.of[3] = 8 | 2; });
  bad_plan("offsets missing", [](Case& c) { c.b.obj_ob_off = nullptr; });
  bad_plan("offsets not from 0", [](Case& c) { c.oo[0] = 1; });
  bad_plan("offsets decrease", [](Case& c) { c.oo[10] = c.oo[9] - 1; });
  bad_plan("ids missing", [](Case& c) { c.b.ob_cluster = nullptr; });
  bad_plan("id negative", [](Case& c) { c.oc[0] = -1; });
  bad_plan("id at C", [](Case& c) { c.oc.back() = 40; });
  bad_plan("ids equal", [](Case& c) { c.oc[c.oo[4] + 1] = c.oc[c.oo[4]]; });
  bad_plan("ids descend", [](Case& c) { c.oc[c.oo[4] + 1] = c.oc[c.oo[4]] - 1 < 0 ? 0 : c.oc[c.oo[4]] - 1; c.oc[c.oo[4]] += 1; });
  bad_plan("ob_flags missing", [](Case& c) { c.b.ob_flags = nullptr; });
  bad_plan("ob flag unknown", [](Case& c) { c.obf[0] = 17; });
  bad_plan("exists and failed", [](Case& c) { c.obf[0] = 9; });
  bad_plan("neither exists nor failed", [](Case& c) { c.obf[0] = 0; });
  bad_plan("deleting without exists", [](Case& c) { c.obf[0] = 8 | 2; });
  bad_plan("adopted without exists", [](Case& c) { c.obf[0] = 8 | 4; });
  {
    Case c = good(40, 30);
    CHECK(kad_deletion_check(nullptr, &c.v) == KAD_EINVAL && kad_deletion_check(&c.b, nullptr) == KAD_EINVAL);
    CHECK(kad_deletion_finish_check(&c.b, nullptr, &c.r) == KAD_EINVAL && kad_deletion_finish_check(&c.b, &c.fv, nullptr) == KAD_EINVAL);
    c.v.out_op = nullptr;
    CHECK(c.plan() == KAD_EINVAL);
    c.bind();
    c.v.obj_first = nullptr;
    CHECK(c.plan() == KAD_EINVAL);
    c.bind();
    c.fv.n_failed_checks = nullptr;
    CHECK(c.finish() == KAD_EINVAL);
  }
  bad_finish("op_ok missing", [](Case& c) { c.r.op_ok = nullptr; });
  bad_finish("op_ok 2", [](Case& c) { c.ok.back() = 2; });
  bad_finish("obj_wait missing", [](Case& c) { c.r.obj_wait = nullptr; });
  bad_finish("obj_wait unknown", [](Case& c) { c.wait[29] = 4; });
  bad_finish("chk_cluster_flags missing", [](Case& c) { c.r.chk_cluster_flags = nullptr; });
  bad_finish("chk cluster flag unknown", [](Case& c) { c.ccf[0] = 32; });
  bad_finish("chk_off missing", [](Case& c) { c.r.chk_off = nullptr; });
  bad_finish("chk_off decreases", [](Case& c) { c.ko[2] = 0; c.ko[1] = 1; });
  bad_finish("chk id at C", [](Case& c) { c.kc[0] = 40; });
  bad_finish("chk ids not ascending", [](Case& c) {
    c.kc.assign({5, 5});
    c.kf.assign({1, 2});
    for (size_t i = 1; i < c.ko.size(); ++i) c.ko[i] = 2;
    c.r.chk_cluster = c.kc.data();
    c.r.chk_flags = c.kf.data();
  });
  bad_finish("chk_flags missing", [](Case& c) { c.r.chk_flags = nullptr; });
  bad_finish("chk flag none", [](Case& c) { c.kf[0] = 0; });
  bad_finish("chk flag two", [](Case& c) { c.kf[0] = 3; });
  bad_finish("chk flag unknown", [](Case& c) { c.kf[0] = 16; });

  // ---- the arena layout of both calls, as deletion_locked declares it
  for (size_t O : {(size_t)1, (size_t)65537}) {
    const size_t C = 1000, B = 10 * O, K = O, pad16 = (16 - C % 16) % 16;
    DeletionDev d{};
    Arena a;
    a.in(d.cluster_flags, (const uint8_t*)nullptr, C, pad16);
    a.in(d.obj_flags, (const uint8_t*)nullptr, O);
    a.in(d.obj_ob_off, (const int32_t*)nullptr, O + 1);
    a.in(d.ob_cluster, (const int32_t*)nullptr, B);
    a.in(d.ob_flags, (const uint8_t*)nullptr, B);
    a.in(d.long_list, (const int32_t*)nullptr, 0);
    a.out(d.n_unready, 2);
    a.in(d.op_ok, (const uint8_t*)nullptr, B);
    a.in(d.chk_off, (const int32_t*)nullptr, O + 1);
    a.in(d.chk_cluster, (const int32_t*)nullptr, K);
    a.in(d.chk_cluster_flags, (const uint8_t*)nullptr, C, pad16);
    a.out(d.n_failed_ops, (int32_t*)nullptr, O);
    std::vector<char> buf(a.total());
    a.place(buf.data());
    CHECK(a.total() % Arena::ALIGN == 0);
    size_t prev_end = 0;
    for (const Arena::Part& p : a.parts()) {
      CHECK(p.at % Arena::ALIGN == 0 && p.at >= prev_end);
      prev_end = p.at + p.bytes;
    }
    CHECK(prev_end <= a.total());
    // the 16-byte reads of both cluster arrays stay inside their parts' slots
    CHECK((const char*)d.cluster_flags + (C + 15) / 16 * 16 <= (const char*)d.obj_flags);
    CHECK((const char*)d.chk_cluster_flags + (C + 15) / 16 * 16 <= (const char*)d.n_failed_ops);
    CHECK((const char*)d.long_list != (const char*)d.n_unready);  // an empty part keeps a slot
    CHECK((const char*)d.ob_cluster + 4 * B <= (const char*)d.ob_flags);
  }
  const DeletionRoute r0 = route_deletion(0, 0, 0, 0, 256);
  CHECK(r0.grid == 0 && r0.long_grid == 0 && r0.width == 1 && r0.lds == 0);
  const DeletionRoute r1 = route_deletion(1000, 1000000, 3, 10000000, 256);
  CHECK(r1.width == 4 && r1.grid == 2048 && r1.long_grid == 1 && r1.stride == 2048 * 64 && r1.lds == 1008 && r1.long_min == 256);
  if (fails) return 1;
  std::printf("ok: deletion checks\n");
  return 0;
}
