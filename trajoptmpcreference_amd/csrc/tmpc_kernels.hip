// Hand-written gfx950 kernels for the QP side of the batched SQP Schur-complement +
// GBD-PCG solve of TrajoptMPCReference (TrajoptMPCReference.py:510-760 and
// GBD-PCG-Python/PCG.py), redesigned for MI355X:
//
//   * per-knot work (forward dynamics, analytic gradients, merit terms) maps
//     one lane to one (problem, knot) -- or (problem, knot, derivative column)
//     -- with the whole rigid-body state in VGPRs (tmpc_device.h);
//   * the PCG solve maps one workgroup to one problem and one lane to one row
//     of the block-tridiagonal Schur complement S; each lane keeps its rows of
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
// (TrajoptPlant.py:313-316); A = I + dt [[0, I], [dqdd_q, dqdd_qd]],
// B = dt [[0], [Minv]] (TrajoptPlant.py:100-108).
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
    if (A) {
      A[r * NX + col] = (r == col ? 1.0 : 0.0) + dt * (col == NJ + r ? 1.0 : 0.0);
      A[(NJ + r) * NX + col] = (NJ + r == col ? 1.0 : 0.0) + dt * acc;
    }
    if (Bm && col < NJ) {
      Bm[r * NJ + col] = 0.0;
      Bm[(NJ + r) * NJ + col] = dt * Mi[r * NJ + col];
    }
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

// In-place Gauss-Jordan inverse of an SPD matrix (no pivoting needed), one
// 16-lane DPP row per matrix, lane r holding row r in a[]: pivot row p is
// broadcast with DPP row_newbcast:p (a VALU move, no LDS round trip), its
// reciprocal taken once.  Exact for diagonal inputs.  All 64 lanes must run it.
template <int P, int NX>
__device__ __forceinline__ void gj_pivot(double (&a)[NX], int r) {
  double pr[NX];
#pragma unroll
  for (int c = 0; c < NX; ++c) pr[c] = dpp_get<0x150 + P, 0xf>(a[c]);
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

template <int P, int NX>
struct GjSweep {
  static __device__ __forceinline__ void run(double (&a)[NX], int r) {
    gj_pivot<P, NX>(a, r);
    GjSweep<P + 1, NX>::run(a, r);
  }
};
template <int NX>
struct GjSweep<NX, NX> {
  static __device__ __forceinline__ void run(double (&)[NX], int) {}
};

// Ghat = (G_k + rho I)^-1 for the three distinct cost Hessian blocks of
// QuadraticCost (Q, QF, R; TrajoptCost.py:71-83); solveKKTSystem_Schur
// adds rho in place and inverts (TrajoptMPCReference.py:419-422).
// One 16-lane group per matrix, one row per lane (GjSweep).
template <int NJ>
__global__ void __launch_bounds__(64) k_ginv(const CostDev* __restrict__ C, PList P, int B,
                                             const double* __restrict__ rho, const int* __restrict__ active,
                                             double* __restrict__ Ginv) {
  constexpr int NX = 2 * NJ;
  const int lane = threadIdx.x & 63;
  const int slot = (blockIdx.x * blockDim.x + threadIdx.x) >> 4;   // one matrix per 16 lanes
  const int r = lane & 15;
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
  GjSweep<0, NX>::run(a, r);
  if (act && r < n) {
    double* out = Ginv + ((size_t)b * 3 + which) * NX * NX;
#pragma unroll
    for (int c = 0; c < NX; ++c)
      if (c < n) out[r * n + c] = a[c];
  }
}

// k_ginv for the wide models (NX > 16): one 32-lane group per matrix, the pivot row
// broadcast by a lane shuffle instead of a 16-lane DPP row; the operations of gj_pivot, pivot by pivot.
template <int P, int NX>
__device__ __forceinline__ void gj_pivot_wide(double (&a)[NX], int r, int base) {
  double pr[NX];
#pragma unroll
  for (int c = 0; c < NX; ++c) pr[c] = __shfl(a[c], base + P, 64);
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
template <int P, int NX>
struct GjSweepWide {
  static __device__ __forceinline__ void run(double (&a)[NX], int r, int base) {
    gj_pivot_wide<P, NX>(a, r, base);
    GjSweepWide<P + 1, NX>::run(a, r, base);
  }
};
template <int NX>
struct GjSweepWide<NX, NX> {
  static __device__ __forceinline__ void run(double (&)[NX], int, int) {}
};
template <int NJ>
__global__ void __launch_bounds__(64) k_ginv_wide(const CostDev* __restrict__ C, PList P, int B,
                                                  const double* __restrict__ rho, const int* __restrict__ active,
                                                  double* __restrict__ Ginv) {
  constexpr int NX = 2 * NJ;
  static_assert(NX <= 32, "one matrix per 32 lanes");
  const int lane = threadIdx.x & 63;
  const int slot = (blockIdx.x * blockDim.x + threadIdx.x) >> 5;   // one matrix per 32 lanes
  const int r = lane & 31, base = lane & 32;
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
  GjSweepWide<0, NX>::run(a, r, base);
  if (act && r < n) {
    double* out = Ginv + ((size_t)b * 3 + which) * NX * NX;
#pragma unroll
    for (int c = 0; c < NX; ++c)
      if (c < n) out[r * n + c] = a[c];
  }
}

// cost-to-go helpers (QuadraticCost.get_currQ, TrajoptCost.py:40-47)
__device__ __forceinline__ bool use_QF(const CostDev* C, int k, int N) {
  return (k == N - 1) || (C->QF_start >= 0 && k >= C->QF_start);
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

// ======================================================================= block-tridiagonal PCG: tmpc_pcg.h

// ---- standalone PCG on given blocks (tmpc_pcg_batch: the PCG class)
template <int NX, int RPL, int MAXT>
__global__ void __launch_bounds__(MAXT) k_pcg(int B, int N, int precond, const double* __restrict__ Sd,
                                              const double* __restrict__ Sl, const double* __restrict__ Su,
                                              const double* __restrict__ gam, const double* __restrict__ guess,
                                              double tol, int max_iter, double* __restrict__ lam,
                                              int* __restrict__ iters, double* __restrict__ trace_nu,
                                              double* __restrict__ trace_res, double* __restrict__ Pd_out) {
  const int b = blockIdx.x;
  extern __shared__ __align__(16) double lds[];
  const int rows = N * NX;
  pcg_lds_clear(lds, N, NX, 1024);
  const PcgLds L = pcg_lds(lds, N, NX, 1024);
  const PcgLane<NX, RPL> ln(threadIdx.x, N);
  const int k = ln.k, K = N - 1;
  PcgRow<NX> R[RPL];
  double bv[RPL];
#pragma unroll
  for (int m = 0; m < RPL; ++m) {
#pragma unroll
    for (int j = 0; j < NX; ++j) R[m].sd[j] = R[m].sl[j] = R[m].su[j] = R[m].pr[j] = 0.0;
    bv[m] = 0.0;
    if (!ln.valid) continue;
    const int i = ln.r(m);
    const double* d = Sd + (((size_t)b * N + k) * NX + i) * NX;
#pragma unroll
    for (int j = 0; j < NX; ++j) R[m].sd[j] = d[j];
    if (k > 0) {
      const double* l = Sl + (((size_t)b * K + (k - 1)) * NX + i) * NX;
#pragma unroll
      for (int j = 0; j < NX; ++j) R[m].sl[j] = l[j];
    }
    if (k < K) {
      if (Su) {
        const double* up = Su + (((size_t)b * K + k) * NX + i) * NX;
#pragma unroll
        for (int j = 0; j < NX; ++j) R[m].su[j] = up[j];
      } else {
        const double* l = Sl + ((size_t)b * K + k) * NX * NX;
#pragma unroll
        for (int j = 0; j < NX; ++j) R[m].su[j] = l[j * NX + i];
      }
    }
    bv[m] = gam[(size_t)b * rows + ln.row(m)];
  }
  pcg_precondition<NX, RPL>(R, precond, ln, N, L.piv, Pd_out ? Pd_out + ((size_t)b * N + k) * NX * NX : nullptr);
  int it_done = 0;
  double xv[RPL];
  pcg_dispatch<NX, RPL>(precond, R, ln, N, L, bv, guess ? guess + (size_t)b * rows : nullptr, tol, max_iter,
                        trace_nu ? trace_nu + (size_t)b * (max_iter + 1) : nullptr,
                        trace_res ? trace_res + (size_t)b * (max_iter + 1) : nullptr, &it_done, xv);
  if (ln.valid) {
#pragma unroll
    for (int m = 0; m < RPL; ++m) lam[(size_t)b * rows + ln.row(m)] = xv[m];
  }
  if (threadIdx.x == 0) iters[b] = it_done;
}

// ======================================================================= fused QP kernel
// One QP of the SQP loop for one problem per workgroup:
//   prologue  Schur blocks (blockwise form of
//             solveKKTSystem_Schur :419-424): each lane computes its rows of
//             S_kk, S_{k,k-1}, S_{k,k+1} and gamma_k straight into registers
//             from A, B (qp_grad), the defects c (qp_fd) and Ghat (ginv),
//             all staged once into LDS with coalesced loads;
//   body      preconditioner + PCG (pcg_precondition / pcg_run);
//   epilogue  dxu = Ghat (g - C^T lambda) (:449-452), with C^T lambda formed
//             once per knot in LDS.
// S and lambda never leave the chip.
// A_k / B_k are read from HBM (L2-resident, shared by the NX lanes of a knot), not staged:
// that keeps k_qp's LDS under 80 KB so two problems' workgroups share a CU.
__host__ __device__ inline size_t qp_stage_doubles(int N, int NX, int NU) {
  const size_t K = N - 1;
  return 3 * (size_t)NX * NX + (size_t)NX * N + (size_t)NU * K;
}

// LDS layout of k_qp: [staging area | lambda] is reused by the PCG buffers
// (which start at 0); the cost gradients g_k = [dx_k^T Q_k, u_k^T R] live past
// both because they must survive the PCG.  In the epilogue the x / u slots of
// the staging area hold C^T lambda.
__host__ __device__ inline size_t qp_g_offset(int N, int NX, int NU, int VR) {
  const size_t a = qp_stage_doubles(N, NX, NU) + (size_t)N * NX;
  const size_t p = pcg_lds_doubles(N, NX, VR);
  return a > p ? a : p;
}

__host__ __device__ inline size_t qp_lds_doubles(int N, int NX, int NU, int VR) {
  return qp_g_offset(N, NX, NU, VR) + (size_t)N * (NX + NU);
}

struct QpStage {
  const double *A, *B;      // global (this problem's A_k, B_k)
  double *G, *x, *u;        // LDS
};

__device__ __forceinline__ QpStage qp_stage(double* lds, int N, int NX, int NU, const double* A, const double* B) {
  QpStage S;
  S.A = A;
  S.B = B;
  S.G = lds;
  S.x = S.G + 3 * NX * NX;
  S.u = S.x + NX * N;
  return S;
}

__device__ __forceinline__ void lds_copy(double* dst, const double* __restrict__ src, int count) {
  for (int e = threadIdx.x; e < count; e += blockDim.x) dst[e] = src[e];
}

// Row i of block k of the Schur complement and gamma_k[i] into R (:419-424):
//   S_kk = -(A G A^T + B G B^T + Ghat_x,k), S_{k,k-1} = A_{k-1} Ghat_x,k-1,
//   S_{k,k+1} = (A_k Ghat_x,k)^T, gamma_k = c_k + [AB Ghat g]_{k-1} - (Ghat_k g_k)_x
// Ghat blocks: the three distinct cost blocks staged in LDS (QuadraticCost,
// no soft limits), or per knot from HBM (PK: soft limits, k_ginv_soft layout)
template <int NJ, bool PK>
struct GhatSrc {
  static constexpr int NX = 2 * NJ, NU = NJ, GS = NX * NX + NU * NU;
  const double* base;
  __device__ __forceinline__ const double* x(const CostDev* C, int k, int N) const {
    return PK ? base + (size_t)k * GS : base + (use_QF(C, k, N) ? NX * NX : 0);
  }
  __device__ __forceinline__ const double* u(int k) const {
    return PK ? base + (size_t)k * GS + NX * NX : base + 2 * NX * NX;
  }
};

// A_k, B_k of the Euler integrator (TrajoptPlant.py:92-108) as k_qp_grad writes them:
//   A_k = [[I, dt I], [dt dqdd_q, I + dt dqdd_qd]],   B_k = [[0], [dt M^-1]].
// Their first NJ rows are structural -- exactly 1, dt and 0 -- so the fused QP kernel reads only the
// bottom NJ rows: a product's chain keeps its order term by term, a structural 1 or dt
// is the same fma, a structural zero term is dropped (fma(0, g, acc) == acc for finite g, up to the
// sign of a zero).  Half of A_k / B_k never leaves HBM for the QP, prologue and epilogue alike.
template <int NJ, bool PK>
__device__ __forceinline__ double qp_schur_row(const CostDev* __restrict__ C, const QpStage& S,
                                               const GhatSrc<NJ, PK>& Gh, const double* __restrict__ g_lds,
                                               double c_ki, int k, int i, int N, double dt, PcgRow<2 * NJ>& R) {
  constexpr int NX = 2 * NJ, NU = NJ;
  const int K = N - 1;
  const double* Gxk = Gh.x(C, k, N);
  const double* gk = g_lds + k * (NX + NU);
  double gam = c_ki;
  {
    double s = 0.0;
#pragma unroll
    for (int j = 0; j < NX; ++j) s += Gxk[i * NX + j] * gk[j];
    gam -= s;
  }
  if (k == 0) {
#pragma unroll
    for (int j = 0; j < NX; ++j) R.sd[j] = -Gxk[i * NX + j];
  } else {
    const int km = k - 1;
    const double* Gxm = Gh.x(C, km, N);
    const double* Gu = Gh.u(km);
    const double* gm = g_lds + km * (NX + NU);
    const double* A = S.A + km * NX * NX;
    const double* Bm = S.B + km * NX * NU;
    // R.sl = row i of A_{k-1} Ghat_{k-1}: a structural row i < NJ is e_i + dt e_{i+NJ}
    if (i < NJ) {
#pragma unroll
      for (int j = 0; j < NX; ++j) R.sl[j] = fma(dt, Gxm[(i + NJ) * NX + j], Gxm[i * NX + j] + 0.0);
    } else {
#pragma unroll
      for (int j = 0; j < NX; ++j) {
        double acc = 0.0;
#pragma unroll
        for (int m = 0; m < NX; ++m) acc += A[i * NX + m] * Gxm[m * NX + j];
        R.sl[j] = acc;
      }
    }
    // row i of B_{k-1} Ghat_u: zero for a structural row
    double BG[NU];
#pragma unroll
    for (int j = 0; j < NU; ++j) BG[j] = 0.0;
    if (i >= NJ) {
#pragma unroll
      for (int j = 0; j < NU; ++j) {
        double acc = 0.0;
#pragma unroll
        for (int m = 0; m < NU; ++m) acc += Bm[i * NU + m] * Gu[m * NU + j];
        BG[j] = acc;
      }
    }
#pragma unroll
    for (int j = 0; j < NX; ++j) {
      double acc;
      if (j < NJ) {   // structural row j of A_{k-1}; row j of B_{k-1} is zero
        acc = fma(R.sl[j + NJ], dt, R.sl[j] + 0.0);
      } else {
        acc = 0.0;
#pragma unroll
        for (int m = 0; m < NX; ++m) acc += R.sl[m] * A[j * NX + m];
#pragma unroll
        for (int m = 0; m < NU; ++m) acc += BG[m] * Bm[j * NU + m];
      }
      R.sd[j] = -(acc + Gxk[i * NX + j]);
    }
    double s = 0.0;
#pragma unroll
    for (int j = 0; j < NX; ++j) s += R.sl[j] * gm[j];
#pragma unroll
    for (int j = 0; j < NU; ++j) s += BG[j] * gm[NX + j];
    gam += s;
  }
  if (k < K) {
    const double* A = S.A + k * NX * NX;
#pragma unroll
    for (int j = 0; j < NX; ++j) {
      double acc;
      if (j < NJ) {
        acc = fma(dt, Gxk[(j + NJ) * NX + i], Gxk[j * NX + i] + 0.0);
      } else {
        acc = 0.0;
#pragma unroll
        for (int m = 0; m < NX; ++m) acc += A[j * NX + m] * Gxk[m * NX + i];
      }
      R.su[j] = acc;
    }
  }
  return gam;
}

// mode: QP_MODE_PCG   prologue + PCG + epilogue (the fused path);
//       QP_MODE_SCHUR prologue only: S blocks and gamma to Sd_out / Sl_out / gam_out
//                     (method S: the direct solve k_btsolve runs next);
//       QP_MODE_DXU   epilogue only, lambda read from lam_out (method S, after k_btsolve).
//       GM: more than 1024 rows -- S and P^-1 rows in HBM (Sg, [B][4][NX/2][rows][2], PcgRowG), two rows
//           per lane, LDS vectors of QP_MAX_ROWS rows.
//       TRK: the state goal of knot k from the goal window gw [B][N][NX] (tmpc_set_reference) in place of C->xg;
//           the fixed-goal instances never touch gw.
template <int NJ, int RPL, int MAXT, bool PK, int MODE, bool GM = false, bool TRK = false>
__global__ void __launch_bounds__(MAXT) k_qp(const CostDev* __restrict__ C, PList P, int B, int N, double dt, int precond,
                                             const double* __restrict__ x, const double* __restrict__ u,
                                             const int* __restrict__ active, const double* __restrict__ Ginv,
                                             const double* __restrict__ Aall, const double* __restrict__ Ball,
                                             const double* __restrict__ cvec, double tol, int max_iter,
                                             int* __restrict__ iters, double* __restrict__ dx,
                                             double* __restrict__ du, double* __restrict__ lam_out,
                                             double* __restrict__ Sd_out, double* __restrict__ Sl_out,
                                             double* __restrict__ gam_out, double* __restrict__ Pd_out,
                                             const double* __restrict__ jsoft, const double* __restrict__ guess,
                                             double* __restrict__ Sg, const double* __restrict__ gw) {
  constexpr int NX = 2 * NJ, NU = NJ;
  constexpr int VR = GM ? QP_MAX_ROWS : 1024;
  if (!P.has(blockIdx.x, B)) return;
  const int b = P.at(blockIdx.x);
  if (!active[b]) return;
  extern __shared__ __align__(16) double lds[];
  const int rows = N * NX;
  const PcgLane<NX, RPL> ln(threadIdx.x, N);
  const int k = ln.k;
  const int K = N - 1;
  const QpStage S = qp_stage(lds, N, NX, NU, Aall + (size_t)b * K * NX * NX, Ball + (size_t)b * K * NX * NU);
  double* lam_lds = S.u + NU * K;
  if (!PK) lds_copy(S.G, Ginv + (size_t)b * 3 * NX * NX, 3 * NX * NX);
  const GhatSrc<NJ, PK> Gh{PK ? Ginv + (size_t)b * N * GhatSrc<NJ, PK>::GS : S.G};
  lds_copy(S.x, x + (size_t)b * NX * N, NX * N);
  lds_copy(S.u, u + (size_t)b * NU * K, NU * K);
  __syncthreads();

  // cost gradients g_k = [(x_k - xg)^T Q_k, u_k^T R] (QuadraticCost.gradient, TrajoptCost.py:58-69)
  double* g_lds = lds + qp_g_offset(N, NX, NU, VR);    // [N][NX + NU]
  for (int e = threadIdx.x; e < N * (NX + NU); e += blockDim.x) {
    const int kk = e / (NX + NU), c = e - kk * (NX + NU);
    double g = 0.0;
    if (c < NX) {
      if (C->kind == COST_EE) { g_lds[e] = PK ? jsoft[(size_t)b * N * (NX + NU) + e] : 0.0; continue; }   // in jsoft
      const double* Qk = use_QF(C, kk, N) ? C->QF : C->Q;
      const double* xg = TRK ? gw + ((size_t)b * N + kk) * NX : C->xg;
#pragma unroll
      for (int m = 0; m < NX; ++m) g += (S.x[m * N + kk] - xg[m]) * Qk[m * NX + c];
    } else if (kk < K) {
#pragma unroll
      for (int m = 0; m < NU; ++m) g += S.u[m * K + kk] * C->R[m * NU + (c - NX)];
    }
    if (PK) g = g + jsoft[(size_t)b * N * (NX + NU) + e];   // soft-limit jacobian (:220-225)
    g_lds[e] = g;
  }
  __syncthreads();

  double xv[RPL];
  if constexpr (MODE == QP_MODE_DXU) {
#pragma unroll
    for (int m = 0; m < RPL; ++m) xv[m] = ln.valid ? lam_out[(size_t)b * rows + ln.row(m)] : 0.0;
    if (threadIdx.x == 0) iters[b] = 0;
  } else {
  PcgRow<NX> R[RPL];
  double bv[RPL];
  // GM: this lane's rows of S / P^-1 in HBM (invalid lanes point at slot m N L and never use it)
  double* const Sgb = GM ? Sg + (size_t)b * 4 * NX * rows : nullptr;
  // storage slot of this lane's row m: lane-major (m N L + lane), so that one wave instruction reads
  // 64 consecutive 16-byte pairs (1 KB, whole lines) whatever the rows' order inside a block
  auto g_at = [&](int q, int m) {
    return Sgb + (size_t)q * NX * rows + 2 * ((size_t)m * N * (NX / RPL) + (size_t)ln.k * (NX / RPL) + ln.i);
  };
  auto g_put = [&](int q, int m, int j, double v) { g_at(q, m)[(size_t)(j >> 1) * 2 * rows + (j & 1)] = v; };
#pragma unroll
  for (int m = 0; m < RPL; ++m) {
#pragma unroll
    for (int j = 0; j < NX; ++j) R[m].sd[j] = R[m].sl[j] = R[m].su[j] = R[m].pr[j] = 0.0;
    bv[m] = 0.0;
    if (!ln.valid) continue;
    const int i = ln.r(m);
    bv[m] = qp_schur_row<NJ, PK>(C, S, Gh, g_lds, cvec[(size_t)b * N * NX + k * NX + i], k, i, N, dt, R[m]);
    if (Sd_out) {
#pragma unroll
      for (int j = 0; j < NX; ++j) Sd_out[(((size_t)b * N + k) * NX + i) * NX + j] = R[m].sd[j];
      if (k > 0) {
#pragma unroll
        for (int j = 0; j < NX; ++j) Sl_out[(((size_t)b * K + k - 1) * NX + i) * NX + j] = R[m].sl[j];
      }
      gam_out[(size_t)b * rows + ln.row(m)] = bv[m];
    }
    if constexpr (GM && MODE == QP_MODE_PCG) {
      // off-diagonal rows to HBM now; the diagonal row stays for the preconditioner
#pragma unroll
      for (int j = 0; j < NX; ++j) {
        g_put(0, m, j, R[m].sd[j]);
        g_put(1, m, j, R[m].sl[j]);
        g_put(2, m, j, R[m].su[j]);
        R[m].sl[j] = R[m].su[j] = 0.0;
      }
    }
  }
  if constexpr (MODE == QP_MODE_SCHUR) {
    if (threadIdx.x == 0) iters[b] = 0;
    return;
  }
  __syncthreads();   // the PCG buffers alias the staging area
  pcg_lds_clear(lds, N, NX, VR);
  const PcgLds L = pcg_lds(lds, N, NX, VR);
  pcg_precondition<NX, RPL>(R, precond, ln, N, L.piv, Pd_out ? Pd_out + ((size_t)b * N + k) * NX * NX : nullptr);
  int it_done = 0;
  // PCG warm start (PCG.update_guess, TrajoptMPCReference.py:439-440): guess [B][N NX] or null
  if constexpr (GM) {
    PcgRowG<NX> RG[RPL];
#pragma unroll
    for (int m = 0; m < RPL; ++m) {
#pragma unroll
      for (int j = 0; j < NX; ++j) RG[m].pr[j] = R[m].pr[j];
      RG[m].sd = GRowRef{g_at(0, m), 2 * rows};
      RG[m].sl = GRowRef{g_at(1, m), 2 * rows};
      RG[m].su = GRowRef{g_at(2, m), 2 * rows};
    }
    pcg_dispatch<NX, RPL>(precond, RG, ln, N, L, bv, guess ? guess + (size_t)b * rows : nullptr, tol, max_iter,
                          nullptr, nullptr, &it_done, xv);
  } else {
    pcg_dispatch<NX, RPL>(precond, R, ln, N, L, bv, guess ? guess + (size_t)b * rows : nullptr, tol, max_iter,
                          nullptr, nullptr, &it_done, xv);
  }
  if (threadIdx.x == 0) iters[b] = it_done;
  }

  // ---- epilogue: dxu = Ghat (g - C^T lambda); Ghat re-staged into LDS
  __syncthreads();
  if (!PK) lds_copy(S.G, Ginv + (size_t)b * 3 * NX * NX, 3 * NX * NX);
  if (ln.valid) {
#pragma unroll
    for (int m = 0; m < RPL; ++m) {
      lam_lds[ln.row(m)] = xv[m];
      if (lam_out && MODE == QP_MODE_PCG) lam_out[(size_t)b * rows + ln.row(m)] = xv[m];
    }
  }
  __syncthreads();
  // C^T lambda per knot: x part lambda_k - A_k^T lambda_{k+1} (terminal: lambda_{N-1}),
  // u part -B_k^T lambda_{k+1}; stored in the (dead) x / u staging slots.  The structural rows m < NJ
  // of A_k (e_m + dt e_{m+NJ}) and B_k (0) are not read (qp_schur_row above): column j of A_k^T lambda
  // starts from its one structural term, lambda_j (j < NJ) or dt lambda_{j-NJ}, as the full chain would.
  double* ctl_x = S.x;   // [N][NX]
  double* ctl_u = S.u;   // [K][NU]
  for (int e = threadIdx.x; e < N * NX + K * NU; e += blockDim.x) {
    if (e < N * NX) {
      const int kk = e / NX, j = e - kk * NX;
      double atl = 0.0;
      if (kk < K) {
        const double* A = S.A + kk * NX * NX;
        const double* l1 = lam_lds + (kk + 1) * NX;
        atl = j < NJ ? l1[j] + 0.0 : fma(dt, l1[j - NJ], 0.0);
#pragma unroll
        for (int m = NJ; m < NX; ++m) atl += A[m * NX + j] * l1[m];
      }
      ctl_x[e] = lam_lds[e] - atl;
    } else {
      const int f = e - N * NX;
      const int kk = f / NU, j = f - kk * NU;
      const double* Bm = S.B + kk * NX * NU;
      const double* l1 = lam_lds + (kk + 1) * NX;
      double btl = 0.0;
#pragma unroll
      for (int m = NJ; m < NX; ++m) btl += Bm[m * NU + j] * l1[m];
      ctl_u[f] = -btl;
    }
  }
  __syncthreads();
  for (int e = threadIdx.x; e < N * NX + K * NU; e += blockDim.x) {
    if (e < N * NX) {
      const int kk = e / NX, i = e - kk * NX;
      const double* Gxk = Gh.x(C, kk, N);
      const double* gk = g_lds + kk * (NX + NU);
      const double* ck = ctl_x + kk * NX;
      double acc = 0.0;
#pragma unroll
      for (int j = 0; j < NX; ++j) acc += Gxk[i * NX + j] * (gk[j] - ck[j]);
      dx[(size_t)b * N * NX + e] = acc;
    } else {
      const int f = e - N * NX;
      const int kk = f / NU, i = f - kk * NU;
      const double* Gu = Gh.u(kk);
      const double* gk = g_lds + kk * (NX + NU) + NX;
      const double* ck = ctl_u + kk * NU;
      double acc = 0.0;
#pragma unroll
      for (int j = 0; j < NU; ++j) acc += Gu[i * NU + j] * (gk[j] - ck[j]);
      du[(size_t)b * K * NU + f] = acc;
    }
  }
}

// ======================================================================= method S: direct block-tridiagonal solve
// solveKKTSystem_Schur with use_PCG = False (TrajoptMPCReference.py:441-446)
// solves S lambda = gamma by np.linalg.solve on the dense S.  S is exactly
// block-tridiagonal and negative definite, so the block
// Thomas recursion needs no pivoting:
//   D_0 = S_00, e_0 = gamma_0;   D_k = S_kk - S_{k,k-1} U_{k-1},  e_k = gamma_k - S_{k,k-1} y_{k-1}
//   [U_k | y_k] = D_k^-1 [S_{k,k+1} | e_k]                         (Gauss-Jordan)
//   lambda_{N-1} = y_{N-1},   lambda_k = y_k - U_k lambda_{k+1}
// One wave per problem, one lane per column of the augmented block
// [D_k | S_{k,k+1} | e_k] (2 NX + 1 <= 64 lanes).  The pivot column is
// broadcast with readlane, so the elimination is register-only; the S_{k,k-1}
// entries are wave-uniform (scalar loads).  U_k and y_k go to a per-problem
// scratch for the back substitution.
template <int NX>
__global__ void __launch_bounds__(64) k_btsolve(int N, const int* __restrict__ active, const double* __restrict__ Sd,
                                                const double* __restrict__ Sl, const double* __restrict__ gam,
                                                double* __restrict__ U, double* __restrict__ Y,
                                                double* __restrict__ lam) {
  static_assert(2 * NX + 1 <= 64, "augmented block must fit one wave");
  const int b = blockIdx.x;
  if (!active[b]) return;
  const int t = threadIdx.x;
  const int K = N - 1;
  const double* sd = Sd + (size_t)b * N * NX * NX;
  const double* sl = Sl + (size_t)b * (K > 0 ? K : 1) * NX * NX;
  const double* gm = gam + (size_t)b * N * NX;
  double* Ub = U + (size_t)b * (K > 0 ? K : 1) * NX * NX;
  double* Yb = Y + (size_t)b * N * NX;
  double a[NX], prev[NX];
#pragma unroll
  for (int r = 0; r < NX; ++r) prev[r] = 0.0;
  for (int k = 0; k < N; ++k) {
#pragma unroll
    for (int r = 0; r < NX; ++r) {
      double v = 0.0;
      if (t < NX)
        v = sd[((size_t)k * NX + r) * NX + t];
      else if (t < 2 * NX)
        v = k < K ? sl[((size_t)k * NX + (t - NX)) * NX + r] : 0.0;   // S_{k,k+1}[r][c] = S_{k+1,k}[c][r]
      else if (t == 2 * NX)
        v = gm[k * NX + r];
      a[r] = v;
    }
    if (k > 0 && (t < NX || t == 2 * NX)) {
      const double* L = sl + (size_t)(k - 1) * NX * NX;   // S_{k,k-1}, wave-uniform
#pragma unroll
      for (int r = 0; r < NX; ++r) {
        double acc = 0.0;
#pragma unroll
        for (int m = 0; m < NX; ++m) acc += L[r * NX + m] * prev[m];
        a[r] -= acc;
      }
    }
#pragma unroll
    for (int p = 0; p < NX; ++p) {
      double f[NX];
#pragma unroll
      for (int r = 0; r < NX; ++r) f[r] = readlane_f64(a[r], p);
      const double inv = 1.0 / f[p];
      a[p] *= inv;
#pragma unroll
      for (int r = 0; r < NX; ++r)
        if (r != p) a[r] -= f[r] * a[p];
    }
    if (t >= NX && t < 2 * NX && k < K) {
#pragma unroll
      for (int r = 0; r < NX; ++r) Ub[((size_t)k * NX + r) * NX + (t - NX)] = a[r];
    }
    if (t == 2 * NX) {
#pragma unroll
      for (int r = 0; r < NX; ++r) Yb[k * NX + r] = a[r];
    }
    // U_k column c moves to lane c for the next D; lane 2 NX keeps y_k
    const int src = t < NX ? t + NX : t;
#pragma unroll
    for (int r = 0; r < NX; ++r) {
      const int lo = __shfl(__double2loint(a[r]), src, 64);
      const int hi = __shfl(__double2hiint(a[r]), src, 64);
      prev[r] = __hiloint2double(hi, lo);
    }
  }
  __threadfence();
  // back substitution, lane r < NX owns row r of lambda_k
  double* lb = lam + (size_t)b * N * NX;
  double lv = (t < NX) ? Yb[K * NX + t] : 0.0;
  if (t < NX) lb[K * NX + t] = lv;
  for (int k = K - 1; k >= 0; --k) {
    double ur[NX];
#pragma unroll
    for (int c = 0; c < NX; ++c) ur[c] = t < NX ? Ub[((size_t)k * NX + t) * NX + c] : 0.0;
    double acc = 0.0;
#pragma unroll
    for (int c = 0; c < NX; ++c) acc += ur[c] * readlane_f64(lv, c);
    lv = (t < NX) ? Yb[k * NX + t] - acc : 0.0;
    if (t < NX) lb[k * NX + t] = lv;
  }
}

int launch_btsolve(hipStream_t s, int nx, const QpArgs& a) {
  switch (nx) {
#define CASE_BT(V)                                                                                                    \
  case V:                                                                                                             \
    hipLaunchKernelGGL((k_btsolve<V>), dim3(a.B), dim3(64), 0, s, a.N, a.active, a.Sd, a.Sl, a.gam, a.U, a.Y, a.lam); \
    return 0;
    CASE_BT(2) CASE_BT(4) CASE_BT(6) CASE_BT(8) CASE_BT(10) CASE_BT(12) CASE_BT(14)
    CASE_BT(16) CASE_BT(18) CASE_BT(20) CASE_BT(22) CASE_BT(24)
#undef CASE_BT
    default: return -2;
  }
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
    if constexpr (2 * NJ > 16)
      hipLaunchKernelGGL((k_ginv_wide<NJ>), TMPC_GRID(B * 3 * 32, 64), 0, s, C, P, B, rho, active, G);
    else
      hipLaunchKernelGGL((k_ginv<NJ>), TMPC_GRID(B * 3 * 16, 64), 0, s, C, P, B, rho, active, G);
  }
  static void qp(hipStream_t s, const QpArgs& a) {
    constexpr int NX = 2 * NJ;
    const int rows = a.N * NX;
    // S / P^-1 rows in HBM (Sg), two rows per lane, up to 1024 lanes (method S past 1024 rows runs the
    // same instance for its prologue / epilogue modes, which never touch Sg)
    const bool gm = !kWide<NJ> && (rows > 1024 || (rows >= qp_gm_min_rows() && a.mode == QP_MODE_PCG));
    const int rpl = gm ? 2 : pcg_rpl(a.N, NX);
    const int threads = ((rows / rpl + 63) / 64) * 64;
    const size_t lds = qp_lds_doubles(a.N, NX, NJ, gm ? QP_MAX_ROWS : 1024) * sizeof(double);
    auto go = [&](auto* kernel) {
      hipLaunchKernelGGL(kernel, dim3(a.B), dim3(threads), lds, s, a.C, a.P, a.B, a.N, a.dt, a.precond, a.x, a.u, a.active,
                         a.G, a.A, a.Bm, a.cvec, a.tol, a.max_iter, a.iters, a.dx, a.du, a.lam, a.Sd, a.Sl, a.gam, a.Pd,
                         a.jsoft, a.guess, a.Sg, a.gw);
    };
#define TMPC_QP_LAUNCH_T(PKV, MODEV, TRKV)                                  \
    if (gm) go(k_qp<NJ, 2, QP_MAX_ROWS / 2, PKV, MODEV, true, TRKV>);       \
    else if (rpl == 1) go(k_qp<NJ, 1, 768, PKV, MODEV, false, TRKV>);       \
    else go(k_qp<NJ, 2, 512, PKV, MODEV, false, TRKV>);
    // a goal window (gw): the tracking instances
#define TMPC_QP_LAUNCH(PKV, MODEV) \
    if (a.gw) { TMPC_QP_LAUNCH_T(PKV, MODEV, true) } else { TMPC_QP_LAUNCH_T(PKV, MODEV, false) }
    if constexpr (kWide<NJ>) {   // a wide model: registers / two rows per lane, no soft limits (launch_qp checks)
#define TMPC_QP_LAUNCH_WT(MODEV, TRKV)                                      \
      if (rpl == 1) go(k_qp<NJ, 1, 768, false, MODEV, false, TRKV>);        \
      else go(k_qp<NJ, 2, 512, false, MODEV, false, TRKV>);
#define TMPC_QP_LAUNCH_W(MODEV) if (a.gw) { TMPC_QP_LAUNCH_WT(MODEV, true) } else { TMPC_QP_LAUNCH_WT(MODEV, false) }
      if (a.mode == QP_MODE_PCG) { TMPC_QP_LAUNCH_W(QP_MODE_PCG) }
      else if (a.mode == QP_MODE_SCHUR) { TMPC_QP_LAUNCH_W(QP_MODE_SCHUR) }
      else { TMPC_QP_LAUNCH_W(QP_MODE_DXU) }
#undef TMPC_QP_LAUNCH_W
#undef TMPC_QP_LAUNCH_WT
    } else {
      // soft limits (jsoft != null): per-knot Ghat from HBM
      if (a.mode == QP_MODE_PCG) {
        if (a.jsoft) { TMPC_QP_LAUNCH(true, QP_MODE_PCG) } else { TMPC_QP_LAUNCH(false, QP_MODE_PCG) }
      } else if (a.mode == QP_MODE_SCHUR) {
        if (a.jsoft) { TMPC_QP_LAUNCH(true, QP_MODE_SCHUR) } else { TMPC_QP_LAUNCH(false, QP_MODE_SCHUR) }
      } else {
        if (a.jsoft) { TMPC_QP_LAUNCH(true, QP_MODE_DXU) } else { TMPC_QP_LAUNCH(false, QP_MODE_DXU) }
      }
    }
#undef TMPC_QP_LAUNCH
#undef TMPC_QP_LAUNCH_T
  }
  static void ginv_soft(hipStream_t s, const GinvSoftArgs& a) {
    const int wpp = (2 * a.N + 4 * GINV_SOFT_GROUPS - 1) / (4 * GINV_SOFT_GROUPS);
    hipLaunchKernelGGL((k_ginv_soft<NJ>), dim3(a.B * wpp), dim3(64), 0, s, a.C, a.Cs, a.P, a.B, a.N, a.rho, a.active, a.x,
                       a.u, a.mu, a.lam, a.Gk, a.jsoft);
  }
};

// the Schur dimensions of the stand-alone PCG (tmpc_pcg_batch): nx = 2, 4, ... 16
constexpr int PCG_NX_MAX = 16;

// set(kernel) for every k_qp instance of NJ joints with (PK) or without the per-knot Ghat of the soft limits
template <int NJ, bool PK, int MD = QP_MODE_PCG, class F>
void for_each_qp(F&& set) {
  if constexpr (MD <= QP_MODE_DXU) {
    set(k_qp<NJ, 1, 768, PK, MD>);
    set(k_qp<NJ, 2, 512, PK, MD>);
    if constexpr (!kWide<NJ>) set(k_qp<NJ, 2, QP_MAX_ROWS / 2, PK, MD, true>);   // S / P^-1 rows in HBM
    set(k_qp<NJ, 1, 768, PK, MD, false, true>);                                  // the tracking instances
    set(k_qp<NJ, 2, 512, PK, MD, false, true>);
    if constexpr (!kWide<NJ>) set(k_qp<NJ, 2, QP_MAX_ROWS / 2, PK, MD, true, true>);
    for_each_qp<NJ, PK, MD + 1>(set);
  }
}

int pcg_set_max_lds() {
  int err = 0;
  auto set = [&](auto* kernel) {
    err |= (int)hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
  };
  for_each_nj<2, PCG_NX_MAX, 2>([&](auto nx) {
    set(k_pcg<decltype(nx)::value, 1, 768>);
    set(k_pcg<decltype(nx)::value, 2, 512>);
  });
  for_each_nj<1, NJMAX>([&](auto nj) {
    constexpr int NJ = decltype(nj)::value;
    for_each_qp<NJ, false>(set);
    if constexpr (!kWide<NJ>) for_each_qp<NJ, true>(set);   // a wide model: no soft limits
  });
  return err;
}

template <int NX>
static void launch_pcg_nx(hipStream_t s, const QpArgs& a) {
  const int rows = a.N * NX;
  const int rpl = pcg_rpl(a.N, NX);
  const int threads = ((rows / rpl + 63) / 64) * 64;
  const size_t lds = pcg_lds_doubles(a.N, NX, 1024) * sizeof(double);
  auto go = [&](auto* kernel) {
    hipLaunchKernelGGL(kernel, dim3(a.B), dim3(threads), lds, s, a.B, a.N, a.precond, a.Sd, a.Sl, a.Su, a.gam, a.guess,
                       a.tol, a.max_iter, a.lam, a.iters, a.tnu, a.tres, a.Pd);
  };
  if (rpl == 1) go(k_pcg<NX, 1, 768>);
  else go(k_pcg<NX, 2, 512>);
}

int launch_pcg(hipStream_t s, int nx, const QpArgs& a) {
  if (a.N * nx > 1024) return -1;
  return for_nj<2, PCG_NX_MAX, 2>(nx, [&](auto v) { launch_pcg_nx<decltype(v)::value>(s, a); });
}


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
int launch_qp(hipStream_t s, int nj, const QpArgs& a) {
  const int rows = a.N * 2 * nj;
  if (rows > QP_MAX_ROWS) return -1;
  if (nj > NJ_FULL && (rows > 1024 || a.jsoft)) return -2;   // a wide model: no HBM-row instance, no soft limits
  const bool gm = nj <= NJ_FULL && (rows > 1024 || (rows >= qp_gm_min_rows() && a.mode == QP_MODE_PCG));
  if (gm && a.mode == QP_MODE_PCG && !a.Sg) return -4;
  if (qp_lds_doubles(a.N, 2 * nj, nj, gm ? QP_MAX_ROWS : 1024) * sizeof(double) > 160 * 1024) return -3;
  return for_nj<1, NJMAX>(nj, [&](auto n) { LaunchNJ<decltype(n)::value>::qp(s, a); });
}
int launch_ginv_soft(hipStream_t s, int nj, const GinvSoftArgs& a) {
  // no soft limits on a wide model
  return for_nj<1, NJ_FULL>(nj, [&](auto n) { LaunchNJ<decltype(n)::value>::ginv_soft(s, a); });
}

}  // namespace tmpc
