// Pure host layout conversions of the C ABI's unit entry points (tmpc_api_qp.cpp): no HIP, no context, so a
// stand-alone program can test them (tests/test_host_pack.py).
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstring>

namespace tmpc {

// The reference's dxul vector per problem: [x_0 u_0 x_1 u_1 ... x_{N-1}] (N nx + (N-1) nu entries), then the
// N nx multipliers.  dx [B][N][nx], du [B][N-1][nu], lam [B][N nx].
inline void pack_dxul(int B, int N, int nx, int nu, const double* dx, const double* du, const double* lam,
                      double* dxul) {
  const int n = nx + nu, K = N - 1;
  const size_t L = (size_t)n * K + nx + (size_t)nx * N;
  for (int b = 0; b < B; ++b) {
    double* o = dxul + b * L;
    for (int k = 0; k < N; ++k) {
      for (int i = 0; i < nx; ++i) o[(size_t)k * n + i] = dx[((size_t)b * N + k) * nx + i];
      if (k < K)
        for (int i = 0; i < nu; ++i) o[(size_t)k * n + nx + i] = du[((size_t)b * K + k) * nu + i];
    }
    memcpy(o + (size_t)n * K + nx, lam + (size_t)b * N * nx, sizeof(double) * N * nx);
  }
}

// The banded QP's multipliers of the N nx dynamics / initial-state rows, in knot order: knot k's rows start
// at roff[b][k] of the problem's dmax-long lambda (its hard rows sit in between).  out [B][N][nx].
inline void gather_dyn_lambda(int B, int N, int nx, int dmax, const int* roff, const double* lam_band, double* out) {
  for (int b = 0; b < B; ++b)
    for (int k = 0; k < N; ++k)
      for (int i = 0; i < nx; ++i)
        out[((size_t)b * N + k) * nx + i] = lam_band[(size_t)b * dmax + roff[(size_t)b * N + k] + i];
}

// M knot-major trajectories [M][n_knots][w] (the iLQR trials on the device) in the trajectory layout of the
// ABI, [M][w][n_knots] (x [nx][N], u [nu][N-1]).
inline void knot_major_to_traj(int M, int n_knots, int w, const double* km, double* traj) {
  for (int m = 0; m < M; ++m)
    for (int k = 0; k < n_knots; ++k)
      for (int i = 0; i < w; ++i)
        traj[((size_t)m * w + i) * n_knots + k] = km[((size_t)m * n_knots + k) * w + i];
}

// The two layouts of a banded S (half-width W, dmax rows, dim[b] <= dmax of them used):
//   ABI    row-major [B][dmax][2W+1]: entry o of row a is column a - W + o
//   device row-start-relative [B][2W+1][dmax]: entry j of row a is column rng[a][0] + j (tmpc_hard.hip), with
//          rng [B][dmax][2] each row's first / last nonzero column -- the range the kernels' products visit
// ABI -> device finds the ranges; device -> ABI is its inverse inside them and writes 0 outside.
inline void band_abi_to_dev(int B, int dmax, int W, const int* dim, const double* S_band, int* rng, double* dev) {
  const size_t BW = 2 * (size_t)W + 1;
  std::fill(dev, dev + (size_t)B * dmax * BW, 0.0);
  for (int b = 0; b < B; ++b)
    for (int a = 0; a < dmax; ++a) {
      const double* row = S_band + ((size_t)b * dmax + a) * BW;
      int lo = a, hi = a;
      for (size_t o = 0; o < BW; ++o) {
        const int c = a - W + (int)o;
        if (c < 0 || c >= dim[b] || row[o] == 0.0) continue;
        lo = std::min(lo, c);
        hi = std::max(hi, c);
      }
      rng[((size_t)b * dmax + a) * 2] = lo;
      rng[((size_t)b * dmax + a) * 2 + 1] = hi;
      for (int c = lo; c <= hi; ++c) dev[((size_t)b * BW + (c - lo)) * dmax + a] = row[c - a + W];
    }
}

inline void band_dev_to_abi(int B, int dmax, int W, const int* dim, const int* rng, const double* dev,
                            double* S_band) {
  const size_t BW = 2 * (size_t)W + 1;
  for (int b = 0; b < B; ++b)
    for (int a = 0; a < dmax; ++a) {
      double* row = S_band + ((size_t)b * dmax + a) * BW;
      const int* r = rng + ((size_t)b * dmax + a) * 2;
      for (size_t o = 0; o < BW; ++o) {
        const int c = a - W + (int)o;
        row[o] = (a >= dim[b] || c < r[0] || c > r[1]) ? 0.0 : dev[((size_t)b * BW + (c - r[0])) * dmax + a];
      }
    }
}

}  // namespace tmpc
