// Stand-alone check of csrc/tmpc_dispatch.h (tests/test_host_dispatch.py compiles and runs it with the host
// compiler's address / undefined-behaviour sanitizers): the table from runtime (model id, joint count, chain,
// precision, QP mode and flags) to template arguments, on three fake compiled models and a recording callable.
#include <cstdio>
#include <type_traits>
#include <vector>

#include "tmpc_dispatch.h"

using namespace tmpc;

static int failures = 0;
#define CHECK(cond)                                            \
  do {                                                         \
    if (!(cond)) {                                             \
      printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); \
      ++failures;                                              \
    }                                                          \
  } while (0)

// model kinds: 0 the runtime model, else the fake's ID
struct Runtime { static constexpr int KIND = 0; };
struct FakeA { static constexpr int KIND = 21, ID = 21, n = 3, chain = 1; };
struct FakeB { static constexpr int KIND = 22, ID = 22, n = 5, chain = 0; };
struct FakeC { static constexpr int KIND = 40, ID = 40, n = 7, chain = 1; };
using Fakes = ModelList<FakeA, FakeB, FakeC>;

struct Hit {
  int nj, chain, kind;
  bool operator==(const Hit& o) const { return nj == o.nj && chain == o.chain && kind == o.kind; }
};

// every call for_model makes for (mid, nj, chain), and its return code
static std::vector<Hit> route(int mid, int nj, bool chain, int* rc) {
  std::vector<Hit> hits;
  *rc = for_model<Runtime>(Fakes{}, mid, nj, chain, [&](auto t) {
    using T = decltype(t);
    hits.push_back({T::nj, T::chain, T::model::KIND});
  });
  return hits;
}

static void check_runtime_table() {
  const int mids[3] = {0, 7, -3};   // no compiled model, and two ids no compiled model has
  for (int mid : mids)
    for (int nj = 1; nj <= 12; ++nj)
      for (int chain = 0; chain <= 1; ++chain) {
        int rc;
        const std::vector<Hit> h = route(mid, nj, chain != 0, &rc);
        CHECK(rc == 0);
        CHECK(h.size() == 1);   // exactly once
        // 8..12 joints: the general-topology instance whatever the model's topology
        const Hit want = {nj, nj <= NJ_FULL ? chain : 0, 0};
        CHECK(h.size() == 1 && h[0] == want);
      }
  for (int nj : {0, 13, -1})
    for (int chain = 0; chain <= 1; ++chain) {
      int rc;
      CHECK(route(0, nj, chain != 0, &rc).empty());
      CHECK(rc == -2);
    }
}

static void check_compiled_models() {
  const Hit want[3] = {{3, 1, 21}, {5, 0, 22}, {7, 1, 40}};
  for (int m = 0; m < 3; ++m)
    for (int nj = -1; nj <= 13; ++nj)   // the model's own n and chain, whatever was passed
      for (int chain = 0; chain <= 1; ++chain) {
        int rc;
        const std::vector<Hit> h = route(want[m].kind, nj, chain != 0, &rc);
        CHECK(rc == 0);
        CHECK(h.size() == 1 && h[0] == want[m]);
      }
  // no compiled model at all: the runtime table alone
  int calls = 0;
  CHECK(for_model<Runtime>(ModelList<>{}, 21, 4, true, [&](auto t) {
          using T = decltype(t);
          calls += T::nj == 4 && T::chain && T::model::KIND == 0;
        }) == 0);
  CHECK(calls == 1);
}

static void check_for_nj() {
  for (int v = -1; v <= 9; ++v) {
    int got = 0, calls = 0;
    const int rc = for_nj<1, 7>(v, [&](auto n) {
      got = decltype(n)::value;
      ++calls;
    });
    if (v >= 1 && v <= 7) {
      CHECK(rc == 0 && calls == 1 && got == v);
    } else {
      CHECK(rc == -2 && calls == 0);   // 8 among them
    }
  }
  // the nx table of the stand-alone PCG: exactly 2, 4, ... 16
  for (int nx = -2; nx <= 19; ++nx) {
    int got = 0, calls = 0;
    const int rc = for_nj<2, 16, 2>(nx, [&](auto n) {
      got = decltype(n)::value;
      ++calls;
    });
    if (nx >= 2 && nx <= 16 && nx % 2 == 0) {
      CHECK(rc == 0 && calls == 1 && got == nx);
    } else {
      CHECK(rc == -2 && calls == 0);
    }
  }
  std::vector<int> seen;
  for_each_nj<1, 12>([&](auto n) { seen.push_back(decltype(n)::value); });
  CHECK(seen == std::vector<int>({1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12}));
  seen.clear();
  for_each_nj<2, 16, 2>([&](auto n) { seen.push_back(decltype(n)::value); });
  CHECK(seen == std::vector<int>({2, 4, 6, 8, 10, 12, 14, 16}));
  seen.clear();
  for_each_nj<3, 2>([&](auto n) { seen.push_back(decltype(n)::value); });
  CHECK(seen.empty());
}

template <int NJ>
static void check_with_real_nj() {
  for (int f32 = 0; f32 <= 1; ++f32) {
    int floats = 0, doubles = 0;
    with_real<NJ>(f32 != 0, [&](auto r) {
      floats += std::is_same<decltype(r), float>::value;
      doubles += std::is_same<decltype(r), double>::value;
    });
    const bool want_float = f32 && NJ <= NJ_FULL;
    CHECK(floats == (want_float ? 1 : 0) && doubles == (want_float ? 0 : 1));
  }
}

static void check_with_real() {
  for_each_nj<1, NJMAX>([](auto n) { check_with_real_nj<decltype(n)::value>(); });
  static_assert(!kWide<NJ_FULL> && kWide<NJ_FULL + 1>, "the wide joint counts start past NJ_FULL");
}

// with_bool / with_qp_mode: a runtime value reaches its one candidate, EVERY all of them in the tables' order
static void check_with_bool() {
  for (int v : {0, 1, 5, EVERY}) {
    std::vector<int> seen;
    with_bool(v, [&](auto b) { seen.push_back(decltype(b)::value ? 1 : 0); });
    if (v == EVERY) CHECK(seen == std::vector<int>({1, 0}));   // true first
    else CHECK(seen == std::vector<int>({v != 0 ? 1 : 0}));
    // an axis without `true` instances: a clear flag and EVERY reach `false` alone, a set flag nothing
    seen.clear();
    with_bool<false>(v, [&](auto b) {
      static_assert(!decltype(b)::value, "with_bool<false> names no true instance");
      seen.push_back(0);
    });
    CHECK(seen == (v > 0 ? std::vector<int>() : std::vector<int>({0})));
  }
}

static void check_with_qp_mode() {
  static_assert(QP_MODE_PCG == 0 && QP_MODE_SCHUR == 1 && QP_MODE_DXU == 2, "QpArgs::mode values");
  for (int mode : {-7, EVERY, 0, 1, 2, 3}) {
    std::vector<int> seen;
    with_qp_mode(mode, [&](auto m) { seen.push_back(decltype(m)::value); });
    if (mode == EVERY) CHECK(seen == std::vector<int>({QP_MODE_PCG, QP_MODE_SCHUR, QP_MODE_DXU}));
    else if (mode >= 0 && mode <= 2) CHECK(seen == std::vector<int>({mode}));
    else CHECK(seen.empty());   // no such mode: no instance
  }
  // the axes nest: every (mode, flag) pair exactly once, and a launch's pair alone
  int pairs[3][2] = {};
  with_qp_mode(EVERY, [&](auto m) { with_bool(EVERY, [&](auto b) { ++pairs[decltype(m)::value][decltype(b)::value]; }); });
  for (auto& row : pairs) CHECK(row[0] == 1 && row[1] == 1);
  int hits = 0;
  with_qp_mode(QP_MODE_SCHUR, [&](auto m) {
    with_bool(1, [&](auto b) { hits += decltype(m)::value == QP_MODE_SCHUR && decltype(b)::value; });
  });
  CHECK(hits == 1);
}

int main() {
  check_runtime_table();
  check_compiled_models();
  check_for_nj();
  check_with_real();
  check_with_bool();
  check_with_qp_mode();
  if (failures) {
    printf("%d check(s) failed\n", failures);
    return 1;
  }
  printf("host dispatch ok\n");
  return 0;
}
