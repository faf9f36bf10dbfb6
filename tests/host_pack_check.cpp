// Stand-alone check of csrc/tmpc_host_pack.h (tests/test_host_pack.py compiles and runs it with the host
// compiler's address / undefined-behaviour sanitizers): pack_dxul against the layout written out by hand, and
// the band round trip ABI -> device -> ABI.
#include <cstdio>
#include <vector>

#include "tmpc_host_pack.h"

static int failures = 0;
#define CHECK(cond)                                            \
  do {                                                         \
    if (!(cond)) {                                             \
      printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); \
      ++failures;                                              \
    }                                                          \
  } while (0)

// dx, du, lam hold distinct tags, so every output entry names its source
static void check_pack_dxul() {
  const int nx = 4, nu = 2, N = 3, B = 2, K = N - 1;
  std::vector<double> dx(B * N * nx), du(B * K * nu), lam(B * N * nx);
  for (size_t i = 0; i < dx.size(); ++i) dx[i] = 1000.0 + i;
  for (size_t i = 0; i < du.size(); ++i) du[i] = 2000.0 + i;
  for (size_t i = 0; i < lam.size(); ++i) lam[i] = 3000.0 + i;
  const size_t L = (nx + nu) * K + nx + nx * N;   // 16 primal entries, 12 multipliers
  CHECK(L == 28);
  std::vector<double> out(B * L, -1.0);
  tmpc::pack_dxul(B, N, nx, nu, dx.data(), du.data(), lam.data(), out.data());
  // problem 0: x_0 u_0 x_1 u_1 x_2 | lambda_0 lambda_1 lambda_2; problem 1 follows, 12 / 4 / 12 tags further on
  const double want0[28] = {1000, 1001, 1002, 1003, 2000, 2001, 1004, 1005, 1006, 1007, 2002, 2003, 1008, 1009,
                            1010, 1011, 3000, 3001, 3002, 3003, 3004, 3005, 3006, 3007, 3008, 3009, 3010, 3011};
  const double want1[28] = {1012, 1013, 1014, 1015, 2004, 2005, 1016, 1017, 1018, 1019, 2006, 2007, 1020, 1021,
                            1022, 1023, 3012, 3013, 3014, 3015, 3016, 3017, 3018, 3019, 3020, 3021, 3022, 3023};
  for (size_t i = 0; i < L; ++i) {
    CHECK(out[i] == want0[i]);
    CHECK(out[L + i] == want1[i]);
  }
}

static void check_gather() {
  // two knots of nx = 2 with one hard row between them: dynamics rows at offsets 0 and 3 of a dmax = 5 lambda
  const int roff[2] = {0, 3};
  const double lam_band[5] = {10, 11, 99, 12, 13};
  double out[4] = {0, 0, 0, 0};
  tmpc::gather_dyn_lambda(1, 2, 2, 5, roff, lam_band, out);
  CHECK(out[0] == 10 && out[1] == 11 && out[2] == 12 && out[3] == 13);
}

static void check_band_round_trip() {
  const int dmax = 7, W = 3, B = 2, BW = 2 * W + 1;
  const int dim[2] = {7, 5};   // problem 1 uses 5 of its 7 rows
  std::vector<double> abi(B * dmax * BW, 0.0);
  auto at = [&](int b, int a, int c) -> double& { return abi[((size_t)b * dmax + a) * BW + (c - a + W)]; };
  for (int b = 0; b < B; ++b)
    for (int a = 0; a < dim[b]; ++a)
      for (int c = a - 2; c <= a + 2; ++c)
        if (c >= 0 && c < dim[b]) at(b, a, c) = 100.0 * (b + 1) + 10.0 * a + c + 0.5;
  // interior zeros: inside a row's first-to-last nonzero range, so they must survive as zeros
  at(0, 3, 2) = 0.0;
  at(0, 3, 4) = 0.0;
  at(1, 2, 2) = 0.0;   // a zero diagonal entry
  at(1, 4, 3) = 0.0;
  // outside what the conversion keeps: past problem 1's dim, and a column past the matrix
  at(1, 4, 5) = 7.0;                              // column 5 >= dim 5
  abi[((size_t)1 * dmax + 6) * BW + W] = 8.0;     // row 6 >= dim 5
  std::vector<int> rng(B * dmax * 2, -1);
  std::vector<double> dev(B * dmax * BW, -1.0), back(B * dmax * BW, -1.0);
  tmpc::band_abi_to_dev(B, dmax, W, dim, abi.data(), rng.data(), dev.data());
  tmpc::band_dev_to_abi(B, dmax, W, dim, rng.data(), dev.data(), back.data());
  for (int b = 0; b < B; ++b)
    for (int a = 0; a < dmax; ++a) {
      const int lo = rng[((size_t)b * dmax + a) * 2], hi = rng[((size_t)b * dmax + a) * 2 + 1];
      CHECK(lo <= a && a <= hi && hi - lo < BW);
      if (a < dim[b]) {
        CHECK(lo == (a - 2 < 0 ? 0 : a - 2));
        CHECK(hi == (a + 2 >= dim[b] ? dim[b] - 1 : a + 2));
      }
      for (int o = 0; o < BW; ++o) {
        const int c = a - W + o;
        const double got = back[((size_t)b * dmax + a) * BW + o];
        const bool inside = a < dim[b] && c >= lo && c <= hi;
        CHECK(got == (inside ? abi[((size_t)b * dmax + a) * BW + o] : 0.0));
      }
    }
  // the device layout itself: entry j of row a at [b][j][a]
  CHECK(dev[((size_t)0 * BW + 0) * dmax + 3] == abi[((size_t)0 * dmax + 3) * BW + (1 - 3 + W)]);   // row 3 starts at column 1
  CHECK(dev[((size_t)0 * BW + 1) * dmax + 3] == 0.0);                                            // its interior zero (column 2)
}

// two knot-major trajectories of 3 knots x 2 entries -> [2][2][3]
static void check_knot_major_to_traj() {
  const double km[12] = {0, 1, 10, 11, 20, 21, 100, 101, 110, 111, 120, 121};   // tag = 100 m + 10 knot + entry
  double out[12];
  for (double& v : out) v = -1.0;
  tmpc::knot_major_to_traj(2, 3, 2, km, out);
  const double want[12] = {0, 10, 20, 1, 11, 21, 100, 110, 120, 101, 111, 121};
  for (int i = 0; i < 12; ++i) CHECK(out[i] == want[i]);
}

int main() {
  check_pack_dxul();
  check_gather();
  check_knot_major_to_traj();
  check_band_round_trip();
  if (failures) return 1;
  printf("host pack ok\n");
  return 0;
}
