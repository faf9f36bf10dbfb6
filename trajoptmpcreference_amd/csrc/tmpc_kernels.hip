// Hand-written gfx950 kernels for the QP side of the batched SQP Schur-complement +
// GBD-PCG solve of TrajoptMPCReference (TrajoptMPCReference.py:510-760 and
// GBD-PCG-Python/PCG.py), redesigned for MI355X.  This file holds what the QP reads: the dynamics
// gradients (k_qp_minv, k_qp_grad, the k_unit_* entry points) and the Ghat inverses (k_ginv, k_ginv_soft);
// the QP solves themselves (k_qp, k_pcg, k_btsolve) are tmpc_qp.hip.
//
//   * per-knot work (forward dynamics, analytic gradients, merit terms) maps
//     one lane to one (problem, knot) -- or (problem, knot, derivative column)
//     -- with the whole rigid-body state in VGPRs (tmpc_device.h);
//   * the PCG solve (tmpc_qp.hip, tmpc_pcg.h) maps one workgroup to one problem and one lane to one
//     row of the block-tridiagonal Schur complement S; each lane keeps its rows of
//     S and of P^-1 in registers for all iterations, vectors are exchanged
//     through LDS and the two dot products per iteration are wave64
//     shuffle reductions + an LDS fan-in (fixed order: deterministic);
//   * per-problem control flow is data, not host branches: every kernel masks itself by
//     the per-problem state, which the solve loops' kernels (tmpc_state.hip) keep.
//
// Layouts (per problem b): x[b][i][k] (nx x N, the reference's column-per-knot
// C order), u[b][i][k] (nu x N-1); per-knot matrices row-major
// [b][k][r][c]; Schur blocks S_diag[b][k][i][j], S_lo[b][k][i][j] = S_{k+1,k}.
#include "tmpc_internal.h"
#include "tmpc_pcg.h"

namespace tmpc {

// ======================================================================= analytic M^-1 columns
// lane = (knot, col), col < NJ; writes the full symmetric matrix (column col
// above the diagonal and row col left of it, :908-930).  x is [K][NX] rows
// with row stride `xstride` per knot and element stride `estride`.
template <int NJ, bool CHAIN, class R, class MT>
__device__ __forceinline__ void minv_lane_store(const MT& M, const double q[NJ], int col,
                                                double* __restrict__ Mo) {
  R cq[NJ], sq[NJ], mc[NJ];
#pragma unroll
  for (int j = 0; j < NJ; ++j) joint_cs(M, j, R(q[j]), cq[j], sq[j]);
  minv_column<NJ, CHAIN>(M, cq, sq, col, mc);
#pragma unroll
  for (int r = 0; r < NJ; ++r) {
    if (r <= col) {
      Mo[r * NJ + col] = double(mc[r]);
      Mo[col * NJ + r] = double(mc[r]);
    }
  }
}

template <int NJ, bool CHAIN, class MT, class R>
__global__ void __launch_bounds__(256) k_qp_minv(MT M, PList P, int B, int N,
                                                 const double* __restrict__ x, const int* __restrict__ need,
                                                 double* __restrict__ minv_out) {
  constexpr int NX = 2 * NJ;
  const int gid = blockIdx.x * blockDim.x + threadIdx.x;
  const int K = N - 1;
  if (gid >= B * K * NJ) return;
  const int col = gid % NJ;
  const int pk = gid / NJ;
  const int p = pk / K, k = pk - p * K;
  if (!P.has(p, B)) return;
  const int b = P.at(p);
  if (!need[b]) return;
  const size_t bk = (size_t)b * K + k;
  const double* xb = x + (size_t)b * NX * N;
  double q[NJ];
#pragma unroll
  for (int j = 0; j < NJ; ++j) q[j] = xb[j * N + k];
  minv_lane_store<NJ, CHAIN, R>(M, q, col, minv_out + (size_t)bk * NJ * NJ);
}

// ======================================================================= gradient columns -> A, B
// lane = (b, k, col), col < 2 NJ.  dqdd[:, col] = -Minv dc[:, col]
// (TrajoptPlant.py:313-316); A and B from it by the integrator section of
// tmpc_device.h (euler_jac_store).
template <int NJ, bool CHAIN, class R, class MT>
__device__ __forceinline__ void grad_lane_store(const MT& M, double dt, const double q[NJ],
                                                const double qd[NJ], const double qdd[NJ],
                                                const double* __restrict__ Mi, int col, double* __restrict__ A,
                                                double* __restrict__ Bm, double* __restrict__ dqdd) {
  constexpr int NX = 2 * NJ;
  R cq[NJ], sq[NJ], dc[NJ], qdr[NJ], qddr[NJ];
#pragma unroll
  for (int j = 0; j < NJ; ++j) {
    joint_cs(M, j, R(q[j]), cq[j], sq[j]);
    qdr[j] = R(qd[j]);
    qddr[j] = R(qdd[j]);
  }
  const bool colqd = col >= NJ;
  rnea_grad_column<NJ, CHAIN>(M, cq, sq, qdr, qddr, colqd ? col - NJ : col, colqd, dc);
#pragma unroll
  for (int r = 0; r < NJ; ++r) {
    R accr = 0.0;
#pragma unroll
    for (int m = 0; m < NJ; ++m) accr += (-R(Mi[r * NJ + m])) * dc[m];
    const double acc = double(accr);
    if (dqdd) {
      dqdd[r * 3 * NJ + col] = acc;
      if (col < NJ) dqdd[r * 3 * NJ + NX + col] = Mi[r * NJ + col];
    }
    euler_jac_store<NJ>(dt, r, col, acc, Mi, A, Bm);
  }
}

template <int NJ, bool CHAIN, class MT, class R>
__global__ void __launch_bounds__(256) k_qp_grad(MT M, PList P, int B, int N, double dt,
                                                 const double* __restrict__ x, const int* __restrict__ need,
                                                 const double* __restrict__ qdd_in, const double* __restrict__ minv_in,
                                                 double* __restrict__ Aout, double* __restrict__ Bout) {
  constexpr int NX = 2 * NJ;
  const int gid = blockIdx.x * blockDim.x + threadIdx.x;
  const int K = N - 1;
  if (gid >= B * K * NX) return;
  const int col = gid % NX;
  const int pk = gid / NX;
  const int p = pk / K, k = pk - p * K;
  if (!P.has(p, B)) return;
  const int b = P.at(p);
  if (!need[b]) return;
  const size_t bk = (size_t)b * K + k;
  const double* xb = x + (size_t)b * NX * N;
  double q[NJ], qd[NJ], qdd[NJ];
#pragma unroll
  for (int j = 0; j < NJ; ++j) {
    q[j] = xb[j * N + k];
    qd[j] = xb[(NJ + j) * N + k];
    qdd[j] = qdd_in[(size_t)bk * NJ + j];
  }
  grad_lane_store<NJ, CHAIN, R>(M, dt, q, qd, qdd, minv_in + (size_t)bk * NJ * NJ, col,
                             Aout + (size_t)bk * NX * NX, Bout + (size_t)bk * NX * NJ, nullptr);
}

// ======================================================================= G-block inverses
// dpp_get: tmpc_pcg.h

// In-place Gauss-Jordan inverse of an SPD matrix (no pivoting needed), one group of W lanes per matrix, lane r
// holding row r in a[]: pivot row p is broadcast and its reciprocal taken once.  W = 16: a DPP row, the
// broadcast is row_newbcast:p (a VALU move, no LDS round trip); W = 32 (the wide models, NX > 16):
// half a wave, a lane shuffle from the group's lane p.  Exact for diagonal inputs.  All 64 lanes must run it.
template <int P, int NX, int W>
__device__ __forceinline__ void gj_pivot(double (&a)[NX], int r) {
  static_assert(W == 16 || W == 32, "a DPP row or half a wave");
  double pr[NX];
#pragma unroll
  for (int c = 0; c < NX; ++c) {
    if constexpr (W == 16) pr[c] = dpp_get<0x150 + P, 0xf>(a[c]);
    else pr[c] = __shfl(a[c], (threadIdx.x & 32) + P, 64);
  }
  const double rp = 1.0 / pr[P];
#pragma unroll
  for (int c = 0; c < NX; ++c) pr[c] *= rp;
  const double f = a[P];
  if (r == P) {
#pragma unroll
    for (int c = 0; c < NX; ++c) a[c] = pr[c];
    a[P] = rp;
  } else {
#pragma unroll
    for (int c = 0; c < NX; ++c) a[c] = fma(-f, pr[c], a[c]);
    a[P] = -f * rp;
  }
}

template <int P, int NX, int W = 16>
struct GjSweep {
  static __device__ __forceinline__ void run(double (&a)[NX], int r) {
    gj_pivot<P, NX, W>(a, r);
    GjSweep<P + 1, NX, W>::run(a, r);
  }
};
template <int NX, int W>
struct GjSweep<NX, NX, W> {
  static __device__ __forceinline__ void run(double (&)[NX], int) {}
};

// Ghat = (G_k + rho I)^-1 for the three distinct cost Hessian blocks of
// QuadraticCost (Q, QF, R; TrajoptCost.py:71-83); solveKKTSystem_Schur
// adds rho in place and inverts (TrajoptMPCReference.py:419-422).
// One group of kGinvLanes<NJ> lanes per matrix, one row per lane (GjSweep).
template <int NJ>
constexpr int kGinvLanes = 2 * NJ > 16 ? 32 : 16;
template <int NJ>
__global__ void __launch_bounds__(64) k_ginv(const CostDev* __restrict__ C, PList P, int B,
                                             const double* __restrict__ rho, const int* __restrict__ active,
                                             double* __restrict__ Ginv) {
  constexpr int NX = 2 * NJ, W = kGinvLanes<NJ>;
  static_assert(NX <= W, "one row per lane");
  const int lane = threadIdx.x & 63;
  const int slot = (blockIdx.x * blockDim.x + threadIdx.x) / W;
  const int r = lane & (W - 1);
  const int ps = slot / 3;
  const bool in_range = slot < B * 3 && P.has(ps, B);
  const int b = in_range ? P.at(ps) : 0, which = in_range ? slot - 3 * ps : 0;
  const bool act = in_range && active[b];
  const int n = which == 2 ? NJ : NX;
  const double* src = which == 0 ? C->Q : (which == 1 ? C->QF : C->R);
  if (!__any(act)) return;   // wave-uniform exit
  const double rh = act ? rho[b] : 0.0;
  double a[NX];
#pragma unroll
  for (int c = 0; c < NX; ++c)
    a[c] = (act && r < n && c < n) ? src[r * n + c] + (r == c ? rh : 0.0) : (r == c ? 1.0 : 0.0);
  GjSweep<0, NX, W>::run(a, r);
  if (act && r < n) {
    double* out = Ginv + ((size_t)b * 3 + which) * NX * NX;
#pragma unroll
    for (int c = 0; c < NX; ++c)
      if (c < n) out[r * n + c] = a[c];
  }
}

// Per-knot Ghat_k = (G_k + rho I)^-1 with soft limits: formKKTSystemBlocks adds
// outer(jac, jac) to the cost Hessian block and jac to its gradient
// (TrajoptMPCReference.py:220-225, :255-259), then solveKKTSystem_Schur adds rho
// (:419-422).  The per-type jacobians have disjoint supports on [q | qd | u], so
// G_k stays block-diagonal in (x, u) and each type's outer product lands in its
// own diagonal sub-block (oracle/soft.py).  One 16-lane group per (problem,
// knot, x|u block), one row per lane, Gauss-Jordan as k_ginv.  Also writes the
// summed jacobian (the g_k increment) to jsoft [B][N][NX + NU].
// Layout of Gk: [B][N][NX*NX + NU*NU] (x block, then the packed u block).
constexpr int GINV_SOFT_GROUPS = 2;
template <int NJ>
__global__ void __launch_bounds__(64) k_ginv_soft(const CostDev* __restrict__ C, const ConstrDev* __restrict__ Cs,
                                                  PList P, int B, int N, const double* __restrict__ rho,
                                                  const int* __restrict__ active, const double* __restrict__ x,
                                                  const double* __restrict__ u, const double* __restrict__ mu,
                                                  const double* __restrict__ lam, double* __restrict__ Gk,
                                                  double* __restrict__ jsoft) {
  constexpr int NX = 2 * NJ, NU = NJ, MC = 6 * NJ;
  // one workgroup per (problem, GINV_SOFT_GROUPS x 4 of its 2N matrices), over the launch's problem list
  // (PList: the lock-step tail no longer dispatches workgroups for problems that have finished, so the
  // groups per workgroup can stay few -- the tail's latency is one workgroup's sequential groups)
  const int lane = threadIdx.x & 63;
  const int r = lane & 15;
  const int wpp = (2 * N + 4 * GINV_SOFT_GROUPS - 1) / (4 * GINV_SOFT_GROUPS);
  const int pb = blockIdx.x / wpp;
  if (pb >= B || !P.has(pb, B)) return;   // workgroup-uniform exit
  const int b = P.at(pb);
  if (!active[b]) return;
  const int c0 = (blockIdx.x - pb * wpp) * 4 * GINV_SOFT_GROUPS;
  for (int grp = 0; grp < GINV_SOFT_GROUPS; ++grp) {
  const int rem = c0 + 4 * grp + (lane >> 4);
  const bool in_range = rem < 2 * N;
  if (!__any(in_range)) break;   // wave-uniform: past the problem's last matrix
  const int k = in_range ? rem >> 1 : 0, which = in_range ? rem & 1 : 0;
  const bool terminal = k == N - 1;
  const bool act = in_range && !(which == 1 && terminal);
  const int n = which ? NJ : NX;
  double z[3 * NJ], jac[3 * NJ];
  const double* xb = x + (size_t)b * NX * N;
  const double* ub = u + (size_t)b * NU * (N - 1);
#pragma unroll
  for (int m = 0; m < NX; ++m) z[m] = act ? xb[m * N + k] : 0.0;
#pragma unroll
  for (int m = 0; m < NU; ++m) z[NX + m] = (act && !terminal) ? ub[m * (N - 1) + k] : 0.0;
  const size_t ko = ((size_t)b * N + k) * MC;
  soft_knot<NJ>(Cs, mu + ko, lam + ko, terminal, z, jac);
  const double* src = which ? C->R : (use_QF(C, k, N) ? C->QF : C->Q);
  const double rh = act ? rho[b] : 0.0;
  // UrdfCost: state-dependent x block (Q Jt)^T Jt (hess_mode 0, TrajoptCost.py:490-492)
  // and its gradient (y^T Q) Jt (:449) joins the soft jacobian in jsoft
  // (2-link only, tmpc_set_cost_ee: compiled out of the other instances, whose registers it would
  // otherwise spill -- k_ginv_soft<6> carried 1168 B/lane of scratch for it)
  const bool ee = NJ == 2 && C->kind == COST_EE && which == 0;
  double eg[NX], hrow[NX];
#pragma unroll
  for (int c = 0; c < NX; ++c) eg[c] = hrow[c] = 0.0;
  if constexpr (NJ == 2) if (ee) {
    double Jt[NX * NX], qj[NX];
    ee_eval<NJ>(C, src, z, eg, Jt);
#pragma unroll
    for (int l = 0; l < NX; ++l) {   // (Q Jt)[l][r]
      double acc = 0.0;
#pragma unroll
      for (int m = 0; m < NX; ++m) {
        double jm = 0.0;
#pragma unroll
        for (int rr = 0; rr < NX; ++rr)
          if (rr == r) jm = Jt[m * NX + rr];
        acc += src[l * NX + m] * jm;
      }
      qj[l] = acc;
    }
#pragma unroll
    for (int c = 0; c < NX; ++c) {
      double acc = 0.0;
#pragma unroll
      for (int l = 0; l < NX; ++l) acc += qj[l] * Jt[l * NX + c];
      hrow[c] = acc;
    }
  }
  double a[NX];
#pragma unroll
  for (int c = 0; c < NX; ++c) {
    double outer = 0.0;
    if (which == 0) {
#pragma unroll
      for (int rr = 0; rr < NX; ++rr)
        if (rr == r && (rr / NJ) == (c / NJ)) outer = jac[rr] * jac[c];
    } else {
#pragma unroll
      for (int rr = 0; rr < NU; ++rr)
        if (rr == r && c < NU) outer = jac[NX + rr] * jac[NX + c];
    }
    const double h = ee ? hrow[c] : src[(r < n ? r : 0) * n + c];
    a[c] = (act && r < n && c < n) ? (h + outer) + (r == c ? rh : 0.0) : (r == c ? 1.0 : 0.0);
  }
  GjSweep<0, NX>::run(a, r);
  if (!in_range || r >= n) continue;
  if (act) {
    double* out = Gk + ((size_t)b * N + k) * (NX * NX + NU * NU) + (which ? NX * NX : 0);
#pragma unroll
    for (int c = 0; c < NX; ++c)
      if (c < n) out[r * n + c] = a[c];
  }
  double jr = 0.0;
#pragma unroll
  for (int m = 0; m < NX; ++m)
    if (m == (which ? NX + r : r)) jr = jac[m];
  if (ee) {
#pragma unroll
    for (int m = 0; m < NX; ++m)
      if (m == r) jr = eg[m] + jr;
  }
  if (which) {
#pragma unroll
    for (int m = 0; m < NU; ++m)
      if (m == r) jr = terminal ? 0.0 : jac[NX + m];
  }
  jsoft[((size_t)b * N + k) * (NX + NU) + (which ? NX : 0) + r] = jr;
  }   // grp
}

// ======================================================================= kernel-level entry points
// [K][nx] / [K][nu] row layout, one lane per knot (or per knot and column)
template <int NJ, bool CHAIN, class MT, class R>
__global__ void __launch_bounds__(256) k_unit_minv(MT M, int K, const double* __restrict__ x,
                                                   double* __restrict__ minv_out) {
  constexpr int NX = 2 * NJ;
  const int gid = blockIdx.x * blockDim.x + threadIdx.x;
  if (gid >= K * NJ) return;
  const int col = gid % NJ, k = gid / NJ;
  double q[NJ];
#pragma unroll
  for (int j = 0; j < NJ; ++j) q[j] = x[(size_t)k * NX + j];
  minv_lane_store<NJ, CHAIN, R>(M, q, col, minv_out + (size_t)k * NJ * NJ);
}

template <int NJ, bool CHAIN, class MT, class R>
__global__ void __launch_bounds__(256) k_unit_grad(MT M, int K, double dt,
                                                   const double* __restrict__ x, const double* __restrict__ qdd_in,
                                                   const double* __restrict__ minv_in, double* __restrict__ Aout,
                                                   double* __restrict__ Bout, double* __restrict__ dqdd) {
  constexpr int NX = 2 * NJ;
  const int gid = blockIdx.x * blockDim.x + threadIdx.x;
  if (gid >= K * NX) return;
  const int col = gid % NX, k = gid / NX;
  double q[NJ], qd[NJ], qdd[NJ];
#pragma unroll
  for (int j = 0; j < NJ; ++j) {
    q[j] = x[(size_t)k * NX + j];
    qd[j] = x[(size_t)k * NX + NJ + j];
    qdd[j] = qdd_in[(size_t)k * NJ + j];
  }
  grad_lane_store<NJ, CHAIN, R>(M, dt, q, qd, qdd, minv_in + (size_t)k * NJ * NJ, col,
                             Aout ? Aout + (size_t)k * NX * NX : nullptr, Bout ? Bout + (size_t)k * NX * NJ : nullptr,
                             dqdd ? dqdd + (size_t)k * NJ * 3 * NJ : nullptr);
}

// ======================================================================= launchers
// f32: the dynamics in fp32 (tmpc_options.precision F32 / MIXED), fp64 in and out
template <int NJ, bool CHAIN, class MT>
struct Launch {
  static void qp_minv(bool f32, hipStream_t s, const ModelDev* M, const DynArgs& a) {
    with_real<NJ>(f32, [&](auto r) {
      hipLaunchKernelGGL((k_qp_minv<NJ, CHAIN, MT, decltype(r)>), TMPC_GRID(a.B * (a.N - 1) * NJ, 256), 0, s, MT::make(M),
                         a.P, a.B, a.N, a.x, a.need, a.minv);
    });
  }
  // a runtime model (ModelRef) takes the general-topology gradient instance even for a chain: with runtime
  // coefficients the chain specialisation's unrolled recursion spills 2.5x more (k_qp_grad<6, chain,
  // ModelRef, double> 4.4 kB per lane against 1.7 kB; 2.7 -> 1.3 ms per headline launch)
  static constexpr bool GCHAIN = MT::STATIC ? CHAIN : false;
  static void qp_grad(bool f32, hipStream_t s, const ModelDev* M, const DynArgs& a) {
    with_real<NJ>(f32, [&](auto r) {
      hipLaunchKernelGGL((k_qp_grad<NJ, GCHAIN, MT, decltype(r)>), TMPC_GRID(a.B * (a.N - 1) * 2 * NJ, 256), 0, s,
                         MT::make(M), a.P, a.B, a.N, a.dt, a.x, a.need, a.qdd, a.minv, a.A, a.Bm);
    });
  }
  static void unit_minv(bool f32, hipStream_t s, const ModelDev* M, const DynArgs& a) {
    with_real<NJ>(f32, [&](auto r) {
      hipLaunchKernelGGL((k_unit_minv<NJ, CHAIN, MT, decltype(r)>), TMPC_GRID(a.K * NJ, 256), 0, s, MT::make(M), a.K, a.x,
                         a.minv);
    });
  }
  static void unit_grad(bool f32, hipStream_t s, const ModelDev* M, const DynArgs& a) {
    with_real<NJ>(f32, [&](auto r) {
      hipLaunchKernelGGL((k_unit_grad<NJ, GCHAIN, MT, decltype(r)>), TMPC_GRID(a.K * 2 * NJ, 256), 0, s, MT::make(M), a.K,
                         a.dt, a.x, a.qdd, a.minv, a.A, a.Bm, a.dqdd);
    });
  }
};

template <int NJ>
struct LaunchNJ {
  static void ginv(hipStream_t s, const CostDev* C, PList P, int B, const double* rho, const int* active, double* G) {
    hipLaunchKernelGGL((k_ginv<NJ>), TMPC_GRID(B * 3 * kGinvLanes<NJ>, 64), 0, s, C, P, B, rho, active, G);
  }
  static void ginv_soft(hipStream_t s, const GinvSoftArgs& a) {
    const int wpp = (2 * a.N + 4 * GINV_SOFT_GROUPS - 1) / (4 * GINV_SOFT_GROUPS);
    hipLaunchKernelGGL((k_ginv_soft<NJ>), dim3(a.B * wpp), dim3(64), 0, s, a.C, a.Cs, a.P, a.B, a.N, a.rho, a.active, a.x,
                       a.u, a.mu, a.lam, a.Gk, a.jsoft);
  }
};

int launch_qp_minv(bool f32, hipStream_t s, const ModelSel& m, const DynArgs& a) {
  return dispatch_model(m.mid, m.nj, m.chain, [&](auto t) {
    using T = decltype(t);
    Launch<T::nj, T::chain, typename T::model>::qp_minv(f32, s, m.M, a);
  });
}
int launch_qp_grad(bool f32, hipStream_t s, const ModelSel& m, const DynArgs& a) {
  return dispatch_model(m.mid, m.nj, m.chain, [&](auto t) {
    using T = decltype(t);
    Launch<T::nj, T::chain, typename T::model>::qp_grad(f32, s, m.M, a);
  });
}
int launch_unit_minv(bool f32, hipStream_t s, const ModelSel& m, const DynArgs& a) {
  return dispatch_model(m.mid, m.nj, m.chain, [&](auto t) {
    using T = decltype(t);
    Launch<T::nj, T::chain, typename T::model>::unit_minv(f32, s, m.M, a);
  });
}
int launch_unit_grad(bool f32, hipStream_t s, const ModelSel& m, const DynArgs& a) {
  return dispatch_model(m.mid, m.nj, m.chain, [&](auto t) {
    using T = decltype(t);
    Launch<T::nj, T::chain, typename T::model>::unit_grad(f32, s, m.M, a);
  });
}
int launch_ginv(hipStream_t s, int nj, const CostDev* C, PList P, int B, const double* rho, const int* active,
                double* G) {
  return for_nj<1, NJMAX>(nj, [&](auto n) { LaunchNJ<decltype(n)::value>::ginv(s, C, P, B, rho, active, G); });
}
int launch_ginv_soft(hipStream_t s, int nj, const GinvSoftArgs& a) {
  // no soft limits on a wide model
  return for_nj<1, NJ_FULL>(nj, [&](auto n) { LaunchNJ<decltype(n)::value>::ginv_soft(s, a); });
}

}  // namespace tmpc
