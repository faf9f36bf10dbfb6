// Per-knot forward-dynamics kernels (one lane per knot): the QP-build
// defects, the line-search merit terms, the unit-test entry point and the
// workload rollout.  Compiled in their own translation unit with the
// register-minimising scheduler (see Makefile): the fully unrolled
// articulated-body recursion for n = 6 otherwise spills to scratch.
#include "tmpc_internal.h"

namespace tmpc {

// ======================================================================= per-knot forward dynamics
// Solver mode: lane = (b, k), k < N-1.  Writes qdd (the point the gradient is
// evaluated at, TrajoptPlant.py:313) and the dynamics defect
// c_{k+1} = x_{k+1} - f(x_k, u_k) (formKKTSystemBlocks :227-231); lane k = 0
// also writes c_0 = x_0 - xs (:213-214).
template <int NJ, bool CHAIN, class MT, class R>
__global__ void __launch_bounds__(256) k_qp_fd(MT M, PList P, int B, int N, double dt,
                                               const double* __restrict__ x, const double* __restrict__ u,
                                               const double* __restrict__ xs, const int* __restrict__ need,
                                               double* __restrict__ qdd_out, double* __restrict__ cvec) {
  constexpr int NX = 2 * NJ;
  const int gid = blockIdx.x * blockDim.x + threadIdx.x;
  const int K = N - 1;
  if (gid >= B * K) return;
  const int p = gid / K, k = gid - p * K;
  if (!P.has(p, B)) return;
  const int b = P.at(p);
  if (!need[b]) return;
  const double* xb = x + (size_t)b * NX * N;
  const double* ub = u + (size_t)b * NJ * K;
  // (state_qdd of tmpc_device.h's integrator section, as text: see profiles/euler_step/README.md)
  double q[NJ], qd[NJ], qdd[NJ];
  R qdr[NJ], ur[NJ], qddr[NJ], cq[NJ], sq[NJ];
#pragma unroll
  for (int j = 0; j < NJ; ++j) {
    q[j] = xb[j * N + k];
    qd[j] = xb[(NJ + j) * N + k];
    qdr[j] = R(qd[j]);
    ur[j] = R(ub[j * K + k]);
    joint_cs(M, j, R(q[j]), cq[j], sq[j]);
  }
  fd_aba<NJ, CHAIN>(M, cq, sq, qdr, ur, qddr);
#pragma unroll
  for (int j = 0; j < NJ; ++j) qdd[j] = double(qddr[j]);
  const size_t kk = (size_t)b * K + k;
#pragma unroll
  for (int j = 0; j < NJ; ++j) qdd_out[kk * NJ + j] = qdd[j];
  double* cb = cvec + (size_t)b * N * NX;
#pragma unroll
  for (int j = 0; j < NJ; ++j) {
    const double xq = euler_next(q[j], dt, qd[j]);
    const double xv = euler_next(qd[j], dt, qdd[j]);
    cb[(k + 1) * NX + j] = xb[j * N + k + 1] - xq;
    cb[(k + 1) * NX + NJ + j] = xb[(NJ + j) * N + k + 1] - xv;
  }
  if (k == 0) {
#pragma unroll
    for (int i = 0; i < NX; ++i) cb[i] = xb[i * N] - xs[(size_t)b * NX + i];
  }
}

// ======================================================================= line-search merit terms
// lane = (b, t, k): for trial step alpha_t evaluate the per-knot pieces of
// totalCost (:296-310), totalHardConstraintViolation (:273-294) and the
// directional derivative D (:635-648, gradient taken at x_new as the
// reference does).  Knot lane N-1 carries the terminal cost / D term and the
// |x_0 - xs| violation term.  SOFT: soft-limit value (slot 3, summed after
// the cost terms as totalCost does, :303-307) and jacobian . dxu added to D
// (:633-646).  terms: [B][T][N][4] = cost, violation, D, soft value.
// Two waves per SIMD (amdgpu_waves_per_eu(2)): left to itself the compiler took 256 VGPRs + 76 AGPRs, one
// wave per SIMD, with nothing to hide the dynamics' latencies; at two it spills 348 B/lane and the headline
// launch takes 0.142 ms instead of 0.195 (profiles/r04/ls_terms).
// TRK: the knot's state goal from the goal window gw [B][N][NX] (tmpc_set_reference) in place of C->xg -- one
// contiguous run per lane whose address depends on (b, k) only, so it is issued with the knot's x / dx loads.
template <int NJ, bool CHAIN, bool SOFT, class MT, class R, bool TRK>
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2))) k_ls_terms(MT M, const CostDev* __restrict__ C,
                                                  const ConstrDev* __restrict__ Cs, const double* __restrict__ mu,
                                                  const double* __restrict__ lam,
                                                  PList P, int B, int N, int T, double dt, const double* __restrict__ alphas,
                                                  const double* __restrict__ x, const double* __restrict__ u,
                                                  const double* __restrict__ xs, const double* __restrict__ dx,
                                                  const double* __restrict__ du, const int* __restrict__ active,
                                                  double* __restrict__ terms, const double* __restrict__ gw) {
  constexpr int NX = 2 * NJ, NU = NJ;
  const int gid = blockIdx.x * blockDim.x + threadIdx.x;
  if (gid >= B * T * N) return;
  const int k = gid % N;
  const int pt = gid / N;
  const int p = pt / T, t = pt - p * T;
  if (!P.has(p, B)) return;
  const int b = P.at(p);
  if (!active[b]) return;
  const size_t bt = (size_t)b * T + t;
  const int K = N - 1;
  const double al = alphas[t];
  const double* xb = x + (size_t)b * NX * N;
  const double* ub = u + (size_t)b * NU * K;
  const double* dxb = dx ? dx + (size_t)b * N * NX : nullptr;
  const double* dub = du ? du + (size_t)b * K * NU : nullptr;
  double xk[NX], dxk[NX];
#pragma unroll
  for (int m = 0; m < NX; ++m) {
    dxk[m] = dxb ? dxb[k * NX + m] : 0.0;
    // x_new = x - alpha dx  (:619-622; alpha is a power of two: exact)
    xk[m] = dxb ? xb[m * N + k] - al * dxk[m] : xb[m * N + k];
  }
  const double* Qk = use_QF(C, k, N) ? C->QF : C->Q;
  double cost, Dk = 0.0;
  if (C->kind == COST_EE) {
    // UrdfCost value and gradient at the trial point (TrajoptCost.py:402-458)
    double gx[NX], Jt[NX * NX];
    cost = ee_eval<NJ>(C, Qk, xk, gx, Jt);
#pragma unroll
    for (int m = 0; m < NX; ++m) Dk += gx[m] * dxk[m];
  } else {
  double d[NX];
  const double* xg = TRK ? gw + ((size_t)b * N + k) * NX : C->xg;
#pragma unroll
  for (int m = 0; m < NX; ++m) d[m] = xk[m] - xg[m];
  // value: 0.5 dx^T (Q dx) [+ 0.5 u^T (R u)]; gradient: [dx^T Q, u^T R]
  double vq = 0.0;
  if (C->diag) {   // the same chains without their exact-zero terms (CostDev.diag)
    const double pz = diag_poison(d, NX);
#pragma unroll
    for (int r = 0; r < NX; ++r) {
      const double qd = __fma_rn(Qk[r * NX + r], d[r], 0.0);
      vq = __fma_rn(d[r], qd, vq);
      Dk = __fma_rn(qd + pz, dxk[r], Dk);
    }
    vq = vq + pz;
  } else {
#pragma unroll
  for (int r = 0; r < NX; ++r) {
    double qd = 0.0, gq = 0.0;
#pragma unroll
    for (int c = 0; c < NX; ++c) {
      qd += Qk[r * NX + c] * d[c];
      gq += d[c] * Qk[c * NX + r];
    }
    vq += d[r] * qd;
    Dk += gq * dxk[r];
  }
  }
  cost = 0.5 * vq;
  }
  double viol = 0.0;
  double* out = terms + ((size_t)bt * N + k) * 4;
  double uk[NU], duk[NU];
#pragma unroll
  for (int m = 0; m < NU; ++m) uk[m] = duk[m] = 0.0;
  if (k < K) {
#pragma unroll
    for (int m = 0; m < NU; ++m) {
      duk[m] = dub ? dub[k * NU + m] : 0.0;
      uk[m] = dub ? ub[m * K + k] - al * duk[m] : ub[m * K + k];
    }
    double vr = 0.0;
    if (C->diag) {
      const double pz = diag_poison(uk, NU);
#pragma unroll
      for (int r = 0; r < NU; ++r) {
        const double ru = __fma_rn(C->R[r * NU + r], uk[r], 0.0);
        vr = __fma_rn(uk[r], ru, vr);
        Dk = __fma_rn(ru + pz, duk[r], Dk);
      }
      vr = vr + pz;
    } else {
#pragma unroll
    for (int r = 0; r < NU; ++r) {
      double ru = 0.0, gr = 0.0;
#pragma unroll
      for (int c = 0; c < NU; ++c) {
        ru += C->R[r * NU + c] * uk[c];
        gr += uk[c] * C->R[c * NU + r];
      }
      vr += uk[r] * ru;
      Dk += gr * duk[r];
    }
    }
    cost += 0.5 * vr;
    // dynamics defect at the trial point
    // (state_qdd of tmpc_device.h's integrator section, as text: see profiles/euler_step/README.md)
    double qd[NJ], qdd[NJ];
    R cq[NJ], sq[NJ], qdr[NJ], ur[NJ], qddr[NJ];
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      qd[j] = xk[NJ + j];
      qdr[j] = R(qd[j]);
      ur[j] = R(uk[j]);
      joint_cs(M, j, R(xk[j]), cq[j], sq[j]);
    }
    fd_aba<NJ, CHAIN>(M, cq, sq, qdr, ur, qddr);
#pragma unroll
    for (int j = 0; j < NJ; ++j) qdd[j] = double(qddr[j]);
#pragma unroll
    for (int m = 0; m < NX; ++m) {
      const double dxn = dxb ? dxb[(k + 1) * NX + m] : 0.0;
      const double xn = dxb ? xb[m * N + k + 1] - al * dxn : xb[m * N + k + 1];
      const double xdot = m < NJ ? qd[m] : qdd[m - NJ];
      const double f = euler_next(xk[m], dt, xdot);
      viol += fabs(xn - f);
    }
  } else {
    // |x_0 - xs|_1 for the initial-state constraint
#pragma unroll
    for (int m = 0; m < NX; ++m) {
      const double x0 = dxb ? xb[m * N] - al * dxb[m] : xb[m * N];
      viol += fabs(x0 - xs[(size_t)b * NX + m]);
    }
  }
  double sv = 0.0;
  if (SOFT) {
    double z[3 * NJ], jac[3 * NJ];
#pragma unroll
    for (int m = 0; m < NX; ++m) z[m] = xk[m];
#pragma unroll
    for (int m = 0; m < NU; ++m) z[NX + m] = uk[m];
    const size_t ko = ((size_t)b * N + k) * 6 * NJ;
    sv = soft_knot<NJ>(Cs, mu + ko, lam + ko, k == K, z, jac);
    double Ds = 0.0;
#pragma unroll
    for (int m = 0; m < NX; ++m) Ds += jac[m] * dxk[m];
#pragma unroll
    for (int m = 0; m < NU; ++m) Ds += jac[NX + m] * duk[m];
    Dk = Dk + Ds;
  }
  out[0] = cost;
  out[1] = viol;
  out[2] = Dk;
  out[3] = sv;
}

// ======================================================================= kernel-level entry points
template <int NJ, bool CHAIN, class MT, class R>
__global__ void __launch_bounds__(256) k_unit_fd(MT M, int K, double dt,
                                                 const double* __restrict__ x, const double* __restrict__ u,
                                                 double* __restrict__ xnext, double* __restrict__ qdd_out) {
  constexpr int NX = 2 * NJ;
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= K) return;
  // (state_qdd of tmpc_device.h's integrator section, as text: see profiles/euler_step/README.md)
  double q[NJ], qd[NJ], qdd[NJ];
  R qdr[NJ], ur[NJ], qddr[NJ], cq[NJ], sq[NJ];
#pragma unroll
  for (int j = 0; j < NJ; ++j) {
    q[j] = x[(size_t)k * NX + j];
    qd[j] = x[(size_t)k * NX + NJ + j];
    qdr[j] = R(qd[j]);
    ur[j] = R(u[(size_t)k * NJ + j]);
    joint_cs(M, j, R(q[j]), cq[j], sq[j]);
  }
  fd_aba<NJ, CHAIN>(M, cq, sq, qdr, ur, qddr);
#pragma unroll
  for (int j = 0; j < NJ; ++j) qdd[j] = double(qddr[j]);
#pragma unroll
  for (int j = 0; j < NJ; ++j) {
    qdd_out[(size_t)k * NJ + j] = qdd[j];
    if (xnext) {
      xnext[(size_t)k * NX + j] = euler_next(q[j], dt, qd[j]);
      xnext[(size_t)k * NX + NJ + j] = euler_next(qd[j], dt, qdd[j]);
    }
  }
}

// sequential Euler rollout, one lane per problem (workload setup: §8d)
template <int NJ, bool CHAIN, class MT, class R>
__global__ void __launch_bounds__(64) k_rollout(MT M, PList P, int B, int N, double dt,
                                                double* __restrict__ x, const double* __restrict__ u,
                                                const int* __restrict__ mask) {
  constexpr int NX = 2 * NJ;
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  if (!P.has(p, B)) return;
  const int b = P.at(p);
  if (mask && !mask[b]) return;
  const int K = N - 1;
  double* xb = x + (size_t)b * NX * N;
  const double* ub = u + (size_t)b * NJ * K;
  double q[NJ], qd[NJ];
#pragma unroll
  for (int j = 0; j < NJ; ++j) { q[j] = xb[j * N]; qd[j] = xb[(NJ + j) * N]; }
  for (int k = 0; k < K; ++k) {
    // (state_qdd of tmpc_device.h's integrator section, as text: see profiles/euler_step/README.md)
    double qdd[NJ];
    R ur[NJ], qdr[NJ], qddr[NJ], cq[NJ], sq[NJ];
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      ur[j] = R(ub[j * K + k]);
      qdr[j] = R(qd[j]);
      joint_cs(M, j, R(q[j]), cq[j], sq[j]);
    }
    fd_aba<NJ, CHAIN>(M, cq, sq, qdr, ur, qddr);
#pragma unroll
    for (int j = 0; j < NJ; ++j) qdd[j] = double(qddr[j]);
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      const double nq = euler_next(q[j], dt, qd[j]);
      const double nv = euler_next(qd[j], dt, qdd[j]);
      q[j] = nq;
      qd[j] = nv;
      xb[j * N + k + 1] = nq;
      xb[(NJ + j) * N + k + 1] = nv;
    }
  }
}

// ======================================================================= MPC advance (oracle/mpc.py, AdvanceArgs)
// Everything the MPC loop does between two horizon solves, one 64-lane workgroup per problem.  Lane 0 applies the
// first control to the plant, x_next = integrator(x_0, u_0): the integrator section of tmpc_device.h in fp64
// (state_qdd<double>'s lines, euler_next), while lane 1 copies the solve's status; then the lanes spread along
// the knots, 64 per chunk, for the warm start's shift (x_k <- x_{k+1}, u_k <- u_{k+1}, last knot kept,
// x_0 <- x_next).  A row shifts in place, so a chunk's last lane reads the element the next chunk's first lane
// writes (64 c + 64): every lane loads its knot k + 1 of all rows -- x, u and the warm lambda's block, which
// shifts by the same rule -- into registers, the workgroup meets at a barrier, then every lane stores to knot k.
// Chunks ascend, so a chunk's stores (knots < 64 c + 64) never reach what a later chunk still has to load
// (knots > 64 c + 64).
// The soft constants: BoxConstraint.shift_soft_constraint_constants(1) (TrajoptConstraint.py:168-176) on the
// [B][N][6n] state, arr[:, :-1] = arr[:, 1:]; arr[:, 1:] = init (the reference's semantics: knot 0 takes knot
// 1's value and every later knot of the slot's span returns to soft_initial; torque limits span N - 1 knots).
// Lane sl < 6 NJ holds slot sl's knot-1 values over the barrier while all lanes write the constants, 64
// consecutive elements per pass.
template <int NJ, bool CHAIN, class MT>
__global__ void __launch_bounds__(64) k_mpc_advance(MT M, AdvanceArgs a) {
  constexpr int NX = 2 * NJ, NU = NJ, MC = 6 * NJ;
  static_assert(MC <= 64, "one lane per soft slot");
  const int b = blockIdx.x, t = threadIdx.x;
  const int N = a.N, K = N - 1;
  double* xb = a.x + (size_t)b * NX * N;
  double* ub = a.u + (size_t)b * NU * K;
  __shared__ double xn[NX];
  if (t == 0) {
    // the simulated plant is fp64 in every precision mode
    // (state_qdd<double> of tmpc_device.h's integrator section, as text: see profiles/euler_step/README.md)
    double q[NJ], qd[NJ], uu[NJ], qdd[NJ], cq[NJ], sq[NJ];
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      q[j] = xb[j * N];
      qd[j] = xb[(NJ + j) * N];
      uu[j] = ub[j * K];
      joint_cs(M, j, q[j], cq[j], sq[j]);
    }
    fd_aba<NJ, CHAIN>(M, cq, sq, qd, uu, qdd);
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      xn[j] = euler_next(q[j], a.dt, qd[j]);
      xn[NJ + j] = euler_next(qd[j], a.dt, qdd[j]);
    }
    if (a.x_out) {
#pragma unroll
      for (int m = 0; m < NX; ++m) a.x_out[((size_t)b * NX + m) * a.x_ld] = xn[m];
    }
    if (a.u_out) {
#pragma unroll
      for (int m = 0; m < NU; ++m) a.u_out[((size_t)b * NU + m) * a.u_ld] = uu[m];
    }
  }
  if (t == 1) {
    if (a.code_out) a.code_out[(size_t)b * a.st_ld] = a.exit_code[b];
    if (a.iter_out) a.iter_out[(size_t)b * a.st_ld] = a.iter[b];
  }
  __syncthreads();
  double* lw = a.lam_warm ? a.lam_warm + (size_t)b * N * NX : nullptr;
  for (int c0 = 0; c0 < K; c0 += 64) {   // (uniform bounds: every lane meets every barrier)
    const int k = c0 + t;
    const bool on = k < K, on_u = k + 1 < K;
    double xv[NX], uv[NU], lv[NX];
    if (on) {
#pragma unroll
      for (int m = 0; m < NX; ++m) xv[m] = xb[m * N + k + 1];
      if (on_u) {
#pragma unroll
        for (int m = 0; m < NU; ++m) uv[m] = ub[m * K + k + 1];
      }
      if (lw) {
#pragma unroll
        for (int m = 0; m < NX; ++m) lv[m] = lw[(size_t)(k + 1) * NX + m];
      }
    }
    __syncthreads();
    if (on) {
#pragma unroll
      for (int m = 0; m < NX; ++m) xb[m * N + k] = k == 0 ? xn[m] : xv[m];
      if (on_u) {
#pragma unroll
        for (int m = 0; m < NU; ++m) ub[m * K + k] = uv[m];
      }
      if (lw) {
#pragma unroll
        for (int m = 0; m < NX; ++m) lw[(size_t)k * NX + m] = lv[m];
      }
    }
  }
  if (a.mu) {
    const size_t off = (size_t)b * N * MC;
    double* arrs[3] = {a.mu + off, a.lam + off, a.phi + off};
    SoftInit si[3];
#pragma unroll
    for (int ty = 0; ty < 3; ++ty) si[ty] = soft_initial(a.Cs, ty);
    double first[3] = {0.0, 0.0, 0.0};
    if (t < MC) {
#pragma unroll
      for (int r = 0; r < 3; ++r) first[r] = arrs[r][MC + t];
    }
    __syncthreads();
    for (int i = MC + t; i < N * MC; i += 64) {
      const int k = i / MC, ty = (i - k * MC) / (2 * NJ);
      if (k < (ty == 2 ? N - 1 : N)) {
        const SoftInit s = ty == 0 ? si[0] : ty == 1 ? si[1] : si[2];
        arrs[0][i] = s.mu;
        arrs[1][i] = s.lam;
        arrs[2][i] = s.phi;
      }
    }
    if (t < MC && (t / (2 * NJ) == 2 ? N - 1 : N) > 1) {
#pragma unroll
      for (int r = 0; r < 3; ++r) arrs[r][t] = first[r];
    }
  }
}

template <int NJ, bool CHAIN, class MT>
struct LaunchFD {
  static void qp_fd(bool f32, hipStream_t s, const ModelDev* M, const DynArgs& a) {
    with_real<NJ>(f32, [&](auto r) {
      hipLaunchKernelGGL((k_qp_fd<NJ, CHAIN, MT, decltype(r)>), TMPC_GRID(a.B * (a.N - 1), 256), 0, s, MT::make(M), a.P,
                         a.B, a.N, a.dt, a.x, a.u, a.xs, a.need, a.qdd, a.cvec);
    });
  }
  // a runtime model (ModelRef) takes the general-topology line-search instance even for a chain: with
  // runtime coefficients the chain specialisation's unrolled recursion spills 9x more (k_ls_terms<6,
  // chain, ModelRef, double> 19 kB per lane against 2.2 kB; 11.2 -> 1.9 ms per headline launch, DESIGN.md
  // 4a); the other FD kernels keep the chain instance, which measured faster for them
  static constexpr bool LCHAIN = MT::STATIC ? CHAIN : false;
  // TRK: the tracking instances (a goal window gw), built in their own translation unit (tmpc_fd_trk.hip)
  template <bool TRK>
  static void ls_terms(bool f32, hipStream_t s, const ModelDev* M, const LsTermsArgs& a) {
#define TMPC_LS(SOFTV, RV)                                                                                          \
    hipLaunchKernelGGL((k_ls_terms<NJ, LCHAIN, SOFTV, MT, RV, TRK>), TMPC_GRID(a.B * a.T * a.N, 256), 0, s, MT::make(M), \
                       a.C, a.Cs, a.mu, a.lam, a.P, a.B, a.N, a.T, a.dt, a.alphas, a.x, a.u, a.xs, a.dx, a.du, a.active, \
                       a.terms, a.gw);
    if constexpr (kWide<NJ>) {   // a wide model: fp64 without soft limits only (check_ready refuses the rest)
      TMPC_LS(false, double)
    } else {
      if (a.mu) { if (f32) { TMPC_LS(true, float) } else { TMPC_LS(true, double) } }
      else { if (f32) { TMPC_LS(false, float) } else { TMPC_LS(false, double) } }
    }
#undef TMPC_LS
  }
  static void unit_fd(bool f32, hipStream_t s, const ModelDev* M, const DynArgs& a) {
    with_real<NJ>(f32, [&](auto r) {
      hipLaunchKernelGGL((k_unit_fd<NJ, CHAIN, MT, decltype(r)>), TMPC_GRID(a.K, 256), 0, s, MT::make(M), a.K, a.dt, a.x,
                         a.u, a.xnext, a.qdd);
    });
  }
  // (the MPC entry points refuse a wide model: no instance)
  static void mpc_advance(hipStream_t s, const ModelDev* M, const AdvanceArgs& a) {
    if constexpr (!kWide<NJ>)
      hipLaunchKernelGGL((k_mpc_advance<NJ, CHAIN, MT>), dim3(a.B), dim3(64), 0, s, MT::make(M), a);
  }
  static void rollout(bool f32, hipStream_t s, const ModelDev* M, const Batch& b, double dt, double* x, const double* u,
                      const int* mask) {
    with_real<NJ>(f32, [&](auto r) {
      hipLaunchKernelGGL((k_rollout<NJ, CHAIN, MT, decltype(r)>), TMPC_GRID(b.B, 64), 0, s, MT::make(M), b.P, b.B, b.N,
                         dt, x, u, mask);
    });
  }
};

#ifdef TMPC_TRK_PART
int launch_ls_terms_trk(bool f32, hipStream_t s, const ModelSel& m, const LsTermsArgs& a) {
  return dispatch_model(m.mid, m.nj, m.chain, [&](auto t) {
    using Tag = decltype(t);
    LaunchFD<Tag::nj, Tag::chain, typename Tag::model>::template ls_terms<true>(f32, s, m.M, a);
  });
}
#else
int launch_qp_fd(bool f32, hipStream_t s, const ModelSel& m, const DynArgs& a) {
  return dispatch_model(m.mid, m.nj, m.chain, [&](auto t) {
    using T = decltype(t);
    LaunchFD<T::nj, T::chain, typename T::model>::qp_fd(f32, s, m.M, a);
  });
}
int launch_ls_terms(bool f32, hipStream_t s, const ModelSel& m, const LsTermsArgs& a) {
  if (a.gw) return launch_ls_terms_trk(f32, s, m, a);
  return dispatch_model(m.mid, m.nj, m.chain, [&](auto t) {
    using Tag = decltype(t);
    LaunchFD<Tag::nj, Tag::chain, typename Tag::model>::template ls_terms<false>(f32, s, m.M, a);
  });
}
int launch_unit_fd(bool f32, hipStream_t s, const ModelSel& m, const DynArgs& a) {
  return dispatch_model(m.mid, m.nj, m.chain, [&](auto t) {
    using T = decltype(t);
    LaunchFD<T::nj, T::chain, typename T::model>::unit_fd(f32, s, m.M, a);
  });
}
int launch_rollout(bool f32, hipStream_t s, const ModelSel& m, const Batch& b, double dt, double* x, const double* u,
                   const int* mask) {
  return dispatch_model(m.mid, m.nj, m.chain, [&](auto t) {
    using T = decltype(t);
    LaunchFD<T::nj, T::chain, typename T::model>::rollout(f32, s, m.M, b, dt, x, u, mask);
  });
}

int launch_mpc_advance(hipStream_t s, const ModelSel& m, const AdvanceArgs& a) {
  if (m.nj > NJ_FULL) return -2;
  return dispatch_model(m.mid, m.nj, m.chain, [&](auto t) {
    using T = decltype(t);
    LaunchFD<T::nj, T::chain, typename T::model>::mpc_advance(s, m.M, a);
  });
}

#endif   // TMPC_TRK_PART

}  // namespace tmpc
