// The block-tridiagonal QP solves of the SQP loop (solveKKTSystem_Schur, TrajoptMPCReference.py:361-455, and
// GBD-PCG-Python/PCG.py) on gfx950: the stand-alone PCG on given blocks (k_pcg), the fused QP kernel (k_qp:
// Schur rows, PCG and dxu in one workgroup per problem) and method S's direct block-tridiagonal solve
// (k_btsolve), with their launchers.  The PCG itself is tmpc_pcg.h; the dynamics gradients and the Ghat
// inverses k_qp reads are tmpc_kernels.hip.  Layouts: tmpc_kernels.hip.
#include "tmpc_internal.h"
#include "tmpc_pcg.h"

namespace tmpc {

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

// A_k, B_k of the integrator as k_qp_grad writes them: euler_jac_store in the integrator section of
// tmpc_device.h.  Their first NJ rows are structural -- exactly 1, dt and 0 -- so the fused QP kernel reads only the
// bottom NJ rows: a product's chain keeps its order term by term, a structural 1 or dt
// is the same fma, a structural zero term is dropped (fma(0, g, acc) == acc for finite g, up to the
// sign of a zero).  Half of A_k / B_k never leaves HBM for the QP, prologue and epilogue alike.
// RT = PcgRowC (a diagonal cost: Ghat_x is diagonal, its off-diagonal entries +-0 from k_ginv): entry j < NJ
// of the S_{k,k+1} row is fma(dt, +-0, +-0 + 0.0) = +0 but for j = i mod NJ, so only that entry (su0) and the
// entries j >= NJ (suh) are formed, by the dense row's expressions.
template <int NJ, bool PK, class RT>
__device__ __forceinline__ double qp_schur_row(const CostDev* __restrict__ C, const QpStage& S,
                                               const GhatSrc<NJ, PK>& Gh, const double* __restrict__ g_lds,
                                               double c_ki, int k, int i, int N, double dt, RT& R) {
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
    if constexpr (RowSuPacked<RT>::value) {
      const int j0 = i < NJ ? i : i - NJ;
      R.su0 = fma(dt, Gxk[(j0 + NJ) * NX + i], Gxk[j0 * NX + i] + 0.0);
    }
#pragma unroll
    for (int j = RowSuPacked<RT>::value ? NJ : 0; j < NX; ++j) {
      double acc;
      if (j < NJ) {
        acc = fma(dt, Gxk[(j + NJ) * NX + i], Gxk[j * NX + i] + 0.0);
      } else {
        acc = 0.0;
#pragma unroll
        for (int m = 0; m < NX; ++m) acc += A[j * NX + m] * Gxk[m * NX + i];
      }
      if constexpr (RowSuPacked<RT>::value) R.suh[j - NJ] = acc;
      else R.su[j] = acc;
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
//       SUC: the S_{k,k+1} rows without their structural zeros (PcgRowC, tmpc_pcg.h) -- a diagonal QuadraticCost
//           without soft limits, register rows; bit for bit the dense instance's results.
template <int NJ, int RPL, int MAXT, bool PK, int MODE, bool GM = false, bool TRK = false, bool SUC = false>
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
  static_assert(!SUC || (MODE == QP_MODE_PCG && !PK && !GM), "PcgRowC: the fused PCG on register rows, one Ghat per cost block");
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
  std::conditional_t<SUC, PcgRowC<NX>, PcgRow<NX>> R[RPL];
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
    if constexpr (SUC) {
      R[m].su0 = 0.0;
#pragma unroll
      for (int j = 0; j < NX; ++j) R[m].sd[j] = R[m].sl[j] = R[m].suh[j >> 1] = R[m].pr[j] = 0.0;
    } else {
#pragma unroll
      for (int j = 0; j < NX; ++j) R[m].sd[j] = R[m].sl[j] = R[m].su[j] = R[m].pr[j] = 0.0;
    }
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

// Which k_qp geometry a QP takes (oracle/canon.py qp_rpl restates this rule).  gm: S / P^-1 rows in HBM (Sg), two
// rows per lane, up to 1024 lanes -- past 1024 rows (method S runs the same instance for its prologue / epilogue
// modes, which never touch Sg) and for the PCG from qp_gm_min_rows() rows on; never on a wide model.
struct QpGeom {
  bool gm;
  int rpl;
};
static QpGeom qp_geom(int nj, int N, int mode) {
  const int rows = N * 2 * nj;
  const bool gm = nj <= NJ_FULL && (rows > 1024 || (rows >= qp_gm_min_rows() && mode == QP_MODE_PCG));
  return {gm, gm ? 2 : pcg_rpl(N, 2 * nj)};
}

// The k_qp instances of NJ joints, once.  f(kernel) for those of the QP mode, the flags pk (per-knot Ghat: soft
// limits) and trk (a goal window: the tracking instances) and the geometry g: a launch's values reach one
// instance, EVERY in place of a value all of that axis (pcg_set_max_lds; rpl EVERY: every geometry).
// A wide model has no soft-limit and no HBM-row instances.  suc: the compressed S_{k,k+1} rows (launch_qp_nj) --
// instances for the fused PCG on register rows without soft limits only; never with gm.
template <int NJ, class F>
void for_qp(int mode, int pk, int trk, int suc, int rpl, bool gm, F&& f) {
  with_qp_mode(mode, [&](auto md) {
    with_bool<!kWide<NJ>>(pk, [&](auto p) {
      with_bool(trk, [&](auto t) {
        constexpr int MD = decltype(md)::value;
        constexpr bool PK = decltype(p)::value, TRK = decltype(t)::value;
        with_bool<MD == QP_MODE_PCG && !PK && !kWide<NJ>>(suc, [&](auto c) {
          constexpr bool SUC = decltype(c)::value;
          if constexpr (!kWide<NJ> && !SUC) {
            if (rpl == EVERY || gm) f(k_qp<NJ, 2, QP_MAX_ROWS / 2, PK, MD, true, TRK>);
          }
          if (rpl == EVERY || (!gm && rpl == 1)) f(k_qp<NJ, 1, 768, PK, MD, false, TRK, SUC>);
          if (rpl == EVERY || (!gm && rpl == 2)) f(k_qp<NJ, 2, 512, PK, MD, false, TRK, SUC>);
        });
      });
    });
  });
}

template <int NJ>
static void launch_qp_nj(hipStream_t s, const QpArgs& a, const QpGeom& g) {
  constexpr int NX = 2 * NJ;
  const int threads = ((a.N * NX / g.rpl + 63) / 64) * 64;
  const size_t lds = qp_lds_doubles(a.N, NX, NJ, g.gm ? QP_MAX_ROWS : 1024) * sizeof(double);
  // a diagonal QuadraticCost (CostDev.diag) makes Ghat_x diagonal: the fused PCG on register rows runs on the
  // S_{k,k+1} rows without their structural zeros (TMPC_GENERIC_COST=1 clears diag: the dense instance)
  const bool suc = a.cost_diag && !a.jsoft && !g.gm && a.mode == QP_MODE_PCG && !kWide<NJ>;
  for_qp<NJ>(a.mode, a.jsoft != nullptr, a.gw != nullptr, suc, g.rpl, g.gm, [&](auto* kernel) {
    hipLaunchKernelGGL(kernel, dim3(a.B), dim3(threads), lds, s, a.C, a.P, a.B, a.N, a.dt, a.precond, a.x, a.u, a.active,
                       a.G, a.A, a.Bm, a.cvec, a.tol, a.max_iter, a.iters, a.dx, a.du, a.lam, a.Sd, a.Sl, a.gam, a.Pd,
                       a.jsoft, a.guess, a.Sg, a.gw);
  });
}

// the Schur dimensions of the stand-alone PCG (tmpc_pcg_batch): nx = 2, 4, ... 16
constexpr int PCG_NX_MAX = 16;

int pcg_set_max_lds() {
  int err = 0;
  auto set = [&](auto* kernel) {
    err |= (int)hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
  };
  for_each_nj<2, PCG_NX_MAX, 2>([&](auto nx) {
    set(k_pcg<decltype(nx)::value, 1, 768>);
    set(k_pcg<decltype(nx)::value, 2, 512>);
  });
  for_each_nj<1, NJMAX>([&](auto nj) { for_qp<decltype(nj)::value>(EVERY, EVERY, EVERY, EVERY, EVERY, false, set); });
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

int launch_qp(hipStream_t s, int nj, const QpArgs& a) {
  const int rows = a.N * 2 * nj;
  if (rows > QP_MAX_ROWS) return -1;
  if (nj > NJ_FULL && (rows > 1024 || a.jsoft)) return -2;   // a wide model: no HBM-row instance, no soft limits
  const QpGeom g = qp_geom(nj, a.N, a.mode);
  if (g.gm && a.mode == QP_MODE_PCG && !a.Sg) return -4;
  if (qp_lds_doubles(a.N, 2 * nj, nj, g.gm ? QP_MAX_ROWS : 1024) * sizeof(double) > 160 * 1024) return -3;
  return for_nj<1, NJMAX>(nj, [&](auto n) { launch_qp_nj<decltype(n)::value>(s, a, g); });
}

}  // namespace tmpc
