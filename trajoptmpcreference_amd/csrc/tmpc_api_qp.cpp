// C ABI (include/tmpc.h): the unit entry points -- dynamics, one QP, one iLQR iteration's sweeps, the plugin-hook
// QPs on caller-formed blocks and the stand-alone PCG solvers.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <vector>

#include "tmpc_ctx.h"
#include "tmpc_host_pack.h"

using namespace tmpc;

namespace {

int pcg_precond_ok(tmpc_ctx* ctx, int precond) {
  if (precond != PRECOND_J && precond != PRECOND_BJ && precond != PRECOND_SS && precond != PRECOND_NONE)
    return fail(ctx, "preconditioner %d: valid are J=1, BJ=2, SS=3, 0=4 (PCG.py:52-55)", precond);
  return 0;
}

// dxul of B problems from the device's dx, du and the host's multipliers lam [B][N nx]
int download_dxul(tmpc_ctx* ctx, int B, int N, int nx, int nu, const double* d_dx, const double* d_du,
                  const double* lam, double* dxul) {
  std::vector<double> dx((size_t)B * N * nx), du((size_t)B * (N - 1) * nu);
  HIP_OK(hipMemcpy(dx.data(), d_dx, dx.size() * sizeof(double), hipMemcpyDeviceToHost));
  HIP_OK(hipMemcpy(du.data(), d_du, du.size() * sizeof(double), hipMemcpyDeviceToHost));
  pack_dxul(B, N, nx, nu, dx.data(), du.data(), lam, dxul);
  return 0;
}

// The plugin-hook QPs (tmpc_qp_blocks_batch, tmpc_qp_blocks_banded_batch) on caller-formed blocks: what both
// check first, and the device copies of the blocks with Ghat = (G_k + rho I)^-1 (k_ghat_full; err: its pivots).
struct HookQp {
  double *G, *Gh, *g, *A, *B, *c, *rho, *dx, *du;
  int *err, *it;
};

int hook_qp_sizes(tmpc_ctx* ctx, const char* what, int B, int N, int nx, int nu) {
  if (B < 1 || N < 2) return fail(ctx, "bad sizes B=%d N=%d (B >= 1, N >= 2)", B, N);
  if (nu < 1 || nu > 7 || nx != 2 * nu)
    return fail(ctx, "%s: nx = %d, nu = %d; the device QP takes nx = 2 nu, 1 <= nu <= 7", what, nx, nu);
  return 0;
}

int hook_qp_upload(tmpc_ctx* ctx, int B, int N, int nx, int nu, const double* G, const double* g, const double* A,
                   const double* Bm, const double* c, const double* rho, HookQp& q) {
  const int n = nx + nu, K = N - 1;
  BUF(double, hb_G, (size_t)B * N * n * n);
  BUF(double, hb_Gh, (size_t)B * N * n * n);
  BUF(double, hb_g, (size_t)B * N * n);
  BUF(double, hb_A, (size_t)B * K * nx * nx);
  BUF(double, hb_B, (size_t)B * K * nx * nu);
  BUF(double, hb_c, (size_t)B * N * nx);
  BUF(double, hb_rho, (size_t)B);
  BUF(int, hb_err, (size_t)B);
  BUF(int, hb_it, (size_t)B);
  BUF(double, hb_dx, (size_t)B * N * nx);
  BUF(double, hb_du, (size_t)B * K * nu);
  q.G = hb_G; q.Gh = hb_Gh; q.g = hb_g; q.A = hb_A; q.B = hb_B; q.c = hb_c; q.rho = hb_rho;
  q.err = hb_err; q.it = hb_it; q.dx = hb_dx; q.du = hb_du;
  HIP_OK(hipMemcpyAsync(hb_G, G, sizeof(double) * B * N * n * n, hipMemcpyHostToDevice, ctx->stream));
  HIP_OK(hipMemcpyAsync(hb_g, g, sizeof(double) * B * N * n, hipMemcpyHostToDevice, ctx->stream));
  HIP_OK(hipMemcpyAsync(hb_A, A, sizeof(double) * B * K * nx * nx, hipMemcpyHostToDevice, ctx->stream));
  HIP_OK(hipMemcpyAsync(hb_B, Bm, sizeof(double) * B * K * nx * nu, hipMemcpyHostToDevice, ctx->stream));
  HIP_OK(hipMemcpyAsync(hb_c, c, sizeof(double) * B * N * nx, hipMemcpyHostToDevice, ctx->stream));
  HIP_OK(hipMemcpyAsync(hb_rho, rho, sizeof(double) * B, hipMemcpyHostToDevice, ctx->stream));
  HIP_OK(hipMemsetAsync(hb_err, 0, sizeof(int) * B, ctx->stream));
  Timed t(ctx, "ghat_full");
  LAUNCH_OK(launch_ghat_full(ctx->stream, nu, B, N, hb_G, hb_rho, hb_Gh, hb_err));
  return 0;
}

int hook_qp_pivots(tmpc_ctx* ctx, int B, const HookQp& q) {
  std::vector<int> err(B);
  HIP_OK(hipMemcpy(err.data(), q.err, sizeof(int) * B, hipMemcpyDeviceToHost));
  for (int b = 0; b < B; ++b)
    if (err[b])
      return fail(ctx, "problem %d: G_k + rho I has a zero or non-finite pivot (singular matrix, the reference's "
                  "np.linalg.inv raises LinAlgError)", b);
  return 0;
}

}  // namespace

extern "C" {

int tmpc_rollout_batch_device(tmpc_ctx* ctx, int B, int N, double dt, double* d_x, const double* d_u) {
  if (!ctx) return -1;
  if (!ctx->has_model) return fail(ctx, "no model");
  if (int rc = wide_ok(ctx, "dynamics")) return rc;
  hipSetDevice(ctx->device);
  LAUNCH_OK(launch_rollout(dyn32(ctx), ctx->stream, model_sel(ctx), Batch{{}, B, N}, dt, d_x, d_u));
  HIP_OK(hipStreamSynchronize(ctx->stream));
  return 0;
}

int tmpc_fd_batch(tmpc_ctx* ctx, int K, double dt, const double* x, const double* u, double* xnext, double* qdd,
                  double* Minv) {
  if (!ctx) return -1;
  if (!ctx->has_model) return fail(ctx, "no model");
  if (int rc = wide_ok(ctx, "dynamics")) return rc;
  if (K < 1) return 0;
  hipSetDevice(ctx->device);
  const int nj = ctx->hmodel.n, nx = 2 * nj;
  BUF(double, u_x, (size_t)K * nx);
  BUF(double, u_u, (size_t)K * nj);
  BUF(double, u_xn, (size_t)K * nx);
  BUF(double, u_qdd, (size_t)K * nj);
  BUF(double, u_minv, (size_t)K * nj * nj);
  HIP_OK(hipMemcpyAsync(u_x, x, sizeof(double) * K * nx, hipMemcpyHostToDevice, ctx->stream));
  HIP_OK(hipMemcpyAsync(u_u, u, sizeof(double) * K * nj, hipMemcpyHostToDevice, ctx->stream));
  DynArgs a{};
  a.K = K; a.dt = dt; a.x = u_x; a.u = u_u; a.xnext = u_xn; a.qdd = u_qdd; a.minv = u_minv;
  LAUNCH_OK(launch_unit_fd(dyn32(ctx), ctx->stream, model_sel(ctx), a));
  if (Minv) LAUNCH_OK(launch_unit_minv(dyn32(ctx), ctx->stream, model_sel(ctx), a));
  HIP_OK(hipStreamSynchronize(ctx->stream));
  if (xnext) HIP_OK(hipMemcpy(xnext, u_xn, sizeof(double) * K * nx, hipMemcpyDeviceToHost));
  if (qdd) HIP_OK(hipMemcpy(qdd, u_qdd, sizeof(double) * K * nj, hipMemcpyDeviceToHost));
  if (Minv) HIP_OK(hipMemcpy(Minv, u_minv, sizeof(double) * K * nj * nj, hipMemcpyDeviceToHost));
  return 0;
}

int tmpc_fd_grad_batch(tmpc_ctx* ctx, int K, double dt, const double* x, const double* u, double* A, double* Bo,
                       double* dqdd) {
  if (!ctx) return -1;
  if (!ctx->has_model) return fail(ctx, "no model");
  if (int rc = wide_ok(ctx, "dynamics")) return rc;
  if (K < 1) return 0;
  hipSetDevice(ctx->device);
  const int nj = ctx->hmodel.n, nx = 2 * nj;
  BUF(double, u_x, (size_t)K * nx);
  BUF(double, u_u, (size_t)K * nj);
  BUF(double, u_qdd, (size_t)K * nj);
  BUF(double, u_minv, (size_t)K * nj * nj);
  BUF(double, u_A, (size_t)K * nx * nx);
  BUF(double, u_B, (size_t)K * nx * nj);
  BUF(double, u_dqdd, (size_t)K * nj * 3 * nj);
  HIP_OK(hipMemcpyAsync(u_x, x, sizeof(double) * K * nx, hipMemcpyHostToDevice, ctx->stream));
  HIP_OK(hipMemcpyAsync(u_u, u, sizeof(double) * K * nj, hipMemcpyHostToDevice, ctx->stream));
  const ModelSel m = model_sel(ctx);
  DynArgs a{};   // no xnext: the accelerations only
  a.K = K; a.x = u_x; a.u = u_u; a.qdd = u_qdd; a.minv = u_minv; a.A = u_A; a.Bm = u_B; a.dqdd = u_dqdd;
  LAUNCH_OK(launch_unit_fd(dyn32(ctx), ctx->stream, m, a));
  LAUNCH_OK(launch_unit_minv(dyn32(ctx), ctx->stream, m, a));
  a.dt = dt;
  LAUNCH_OK(launch_unit_grad(dyn32(ctx), ctx->stream, m, a));
  HIP_OK(hipStreamSynchronize(ctx->stream));
  if (A) HIP_OK(hipMemcpy(A, u_A, sizeof(double) * K * nx * nx, hipMemcpyDeviceToHost));
  if (Bo) HIP_OK(hipMemcpy(Bo, u_B, sizeof(double) * K * nx * nj, hipMemcpyDeviceToHost));
  if (dqdd) HIP_OK(hipMemcpy(dqdd, u_dqdd, sizeof(double) * K * nj * 3 * nj, hipMemcpyDeviceToHost));
  return 0;
}

int tmpc_qp_batch(tmpc_ctx* ctx, int B, int N, double dt, int linsys, const double* rho, const double* x,
                  const double* u, const double* xs, const double* guess, double* dxul, int32_t* pcg_iters,
                  double* S_diag, double* S_lo, double* gamma, double* P_diag) {
  if (!ctx) return -1;
  int rc = check_ready(ctx, B, N);
  if (rc) return rc;
  if (ctx->hcost.kind != COST_QUADRATIC) return fail(ctx, "tmpc_qp_batch supports QuadraticCost only");
  const bool banded = qp_banded(ctx, N);
  if (banded && guess)
    return fail(ctx, "tmpc_qp_batch: no PCG guess on the banded path (hard box constraints, or N * nx past %d)",
                QP_MAX_ROWS);
  if (banded && (S_diag || S_lo || gamma || P_diag))
    return fail(ctx, "tmpc_qp_batch: on the banded path (hard box constraints, or N * nx past %d) S is banded; "
                     "S_diag / S_lo / gamma / P_diag must be NULL (tmpc_qp_hard_info has S_band)", QP_MAX_ROWS);
  const int precond = precond_of(linsys);
  if (precond < 0) return fail(ctx, "linear system method %d is not available on the GPU", linsys);
  if (!rho || !x || !u) return fail(ctx, "null input");
  hipSetDevice(ctx->device);
  const int nj = ctx->hmodel.n, nx = 2 * nj, K = N - 1;
  Work w;
  if ((rc = alloc_work(ctx, B, N, w, true))) return rc;
  ProbState st;
  if ((rc = alloc_state(ctx, B, st))) return rc;
  BUF(double, io_x, (size_t)B * nx * N);
  BUF(double, io_u, (size_t)B * nj * K);
  HIP_OK(hipMemcpyAsync(io_x, x, sizeof(double) * B * nx * N, hipMemcpyHostToDevice, ctx->stream));
  HIP_OK(hipMemcpyAsync(io_u, u, sizeof(double) * B * nj * K, hipMemcpyHostToDevice, ctx->stream));
  HIP_OK(hipMemcpyAsync(st.rho, rho, sizeof(double) * B, hipMemcpyHostToDevice, ctx->stream));
  ProbState st0 = st;   // the initial state of a solve, but for rho: the caller's
  st0.rho = st.drho;
  launch_init_state(ctx->stream, B, 0.0, st0);
  if (xs)   // the SQP's initial state (solveKKTSystem_Schur's xs argument, :361): c_0 = x_0 - xs
    HIP_OK(hipMemcpyAsync(w.xs, xs, sizeof(double) * B * nx, hipMemcpyHostToDevice, ctx->stream));
  else
    HIP_OK(hipMemcpy2DAsync(w.xs, sizeof(double), io_x, (size_t)N * sizeof(double), sizeof(double), (size_t)B * nx,
                            hipMemcpyDeviceToDevice, ctx->stream));
  if (guess && precond != 0) {
    BUF(double, io_guess, (size_t)B * N * nx);
    HIP_OK(hipMemcpyAsync(io_guess, guess, sizeof(double) * B * N * nx, hipMemcpyHostToDevice, ctx->stream));
    w.guess = io_guess;
  }
  // soft limits: the QP of formKKTSystemBlocks carries their jacobian terms (:220-225, :255-259) at the
  // context's soft state (tmpc_set_soft_state; defaults if it was never set for this B, N)
  if (ctx->hlim.any && (rc = init_soft(ctx, B, N, false, &w))) return rc;
  // hard box constraints: the QP with the knots' constraint rows (tmpc_hard.hip); the lambda part of
  // dxul then holds the multipliers of the N nx dynamics / initial-state rows, in knot order
  HardArgs hard{};
  if (banded) {
    if ((rc = setup_hard(ctx, B, N, 0, precond, hard))) return rc;
    w.hard = &hard;
  }
  ctx->hard_last = {0, 0, 0, 0, 0};
  if ((rc = goal_window(ctx, B, N, B, "batch size", nullptr, 0, nullptr, &w.qp.gw))) return rc;   // tmpc_set_reference
  bind_work(ctx, N, dt, io_x, io_u, st, w);
  if ((rc = run_qp(ctx, B, precond, st, w, !banded, PList{}, B))) return rc;
  HIP_OK(hipStreamSynchronize(ctx->stream));
  if (banded) {
    if ((rc = collect_hard_work(ctx, hard))) return rc;
    ctx->hard_last = {B, N, hard.dmax, hard.W, hard.rmax};
    std::vector<int> roff((size_t)B * N);
    std::vector<double> lh((size_t)B * hard.dmax);
    HIP_OK(hipMemcpy(roff.data(), hard.roff, roff.size() * sizeof(int), hipMemcpyDeviceToHost));
    HIP_OK(hipMemcpy(lh.data(), hard.lam, lh.size() * sizeof(double), hipMemcpyDeviceToHost));
    std::vector<double> lr((size_t)B * N * nx);
    gather_dyn_lambda(B, N, nx, hard.dmax, roff.data(), lh.data(), lr.data());
    HIP_OK(hipMemcpy(w.lam, lr.data(), lr.size() * sizeof(double), hipMemcpyHostToDevice));
  }
  resolve_timings(ctx);
  ctx->qp_last = {B, N, nj, ctx->hcost.QF_start, w.qp.jsoft != nullptr, banded};   // tmpc_qp_last_inputs
  if (dxul) {
    std::vector<double> lam((size_t)B * N * nx);
    HIP_OK(hipMemcpy(lam.data(), w.lam, lam.size() * sizeof(double), hipMemcpyDeviceToHost));
    if ((rc = download_dxul(ctx, B, N, nx, nj, w.qp.dx, w.qp.du, lam.data(), dxul))) return rc;
  }
  if (pcg_iters) HIP_OK(hipMemcpy(pcg_iters, w.qp.iters, sizeof(int) * B, hipMemcpyDeviceToHost));
  if (S_diag) HIP_OK(hipMemcpy(S_diag, w.Sd, sizeof(double) * B * N * nx * nx, hipMemcpyDeviceToHost));
  if (S_lo) HIP_OK(hipMemcpy(S_lo, w.Sl, sizeof(double) * B * K * nx * nx, hipMemcpyDeviceToHost));
  if (gamma) HIP_OK(hipMemcpy(gamma, w.gam, sizeof(double) * B * N * nx, hipMemcpyDeviceToHost));
  if (P_diag && precond != PRECOND_J && precond != 0)
    HIP_OK(hipMemcpy(P_diag, w.Pd, sizeof(double) * B * N * nx * nx, hipMemcpyDeviceToHost));
  return 0;
}

int tmpc_qp_last_inputs(tmpc_ctx* ctx, int B, int N, double* A, double* Bm, double* c, double* Ghat_x,
                        double* Ghat_u) {
  if (!ctx) return -1;
  const auto& ql = ctx->qp_last;
  if (ql.B == 0)
    return fail(ctx, "tmpc_qp_last_inputs: no tmpc_qp_batch call to report (none yet, or a later call reused its "
                "buffers)");
  if (ql.B != B || ql.N != N)
    return fail(ctx, "tmpc_qp_last_inputs: the last tmpc_qp_batch was B=%d N=%d, asked for B=%d N=%d", ql.B, ql.N, B, N);
  if (ql.banded)
    return fail(ctx, "tmpc_qp_last_inputs: the last tmpc_qp_batch took the banded path (hard box limits, or N * nx "
                "past %d rows); tmpc_qp_hard_info has its detail", QP_MAX_ROWS);
  hipSetDevice(ctx->device);
  const int nj = ql.nj, nx = 2 * nj, K = N - 1;
  // the named buffers of that call (alloc_work, init_soft): the same sizes, so nothing is reallocated
  BUF(double, cvec, (size_t)B * N * nx);
  BUF(double, Amat, (size_t)B * K * nx * nx);
  BUF(double, Bmat, (size_t)B * K * nx * nj);
  if (A) HIP_OK(hipMemcpy(A, Amat, sizeof(double) * B * K * nx * nx, hipMemcpyDeviceToHost));
  if (Bm) HIP_OK(hipMemcpy(Bm, Bmat, sizeof(double) * B * K * nx * nj, hipMemcpyDeviceToHost));
  if (c) HIP_OK(hipMemcpy(c, cvec, sizeof(double) * B * N * nx, hipMemcpyDeviceToHost));
  if (!Ghat_x && !Ghat_u) return 0;
  const size_t XX = (size_t)nx * nx, UU = (size_t)nj * nj;
  if (ql.soft) {   // k_ginv_soft: [B][N][nx nx + nu nu], the u block of the terminal knot unused
    BUF(double, soft_Gk, (size_t)B * N * (XX + UU));
    std::vector<double> h((size_t)B * N * (XX + UU));
    HIP_OK(hipMemcpy(h.data(), soft_Gk, h.size() * sizeof(double), hipMemcpyDeviceToHost));
    for (size_t b = 0; b < (size_t)B; ++b)
      for (size_t k = 0; k < (size_t)N; ++k) {
        const double* s = h.data() + (b * N + k) * (XX + UU);
        if (Ghat_x) memcpy(Ghat_x + (b * N + k) * XX, s, XX * sizeof(double));
        if (Ghat_u && k < (size_t)K) memcpy(Ghat_u + (b * K + k) * UU, s + XX, UU * sizeof(double));
      }
    return 0;
  }
  // k_ginv: [B][3][nx nx] = (Q + rho I)^-1, (QF + rho I)^-1, (R + rho I)^-1 packed at stride nu; knot k reads the
  // QF block at the terminal knot and from QF_start on (use_QF)
  BUF(double, Ginv, (size_t)B * 3 * XX);
  std::vector<double> h((size_t)B * 3 * XX);
  HIP_OK(hipMemcpy(h.data(), Ginv, h.size() * sizeof(double), hipMemcpyDeviceToHost));
  for (size_t b = 0; b < (size_t)B; ++b)
    for (size_t k = 0; k < (size_t)N; ++k) {
      const bool qf = (int)k == N - 1 || (ql.QF_start >= 0 && (int)k >= ql.QF_start);
      if (Ghat_x) memcpy(Ghat_x + (b * N + k) * XX, h.data() + (b * 3 + (qf ? 1 : 0)) * XX, XX * sizeof(double));
      if (Ghat_u && k < (size_t)K) memcpy(Ghat_u + (b * K + k) * UU, h.data() + (b * 3 + 2) * XX, UU * sizeof(double));
    }
  return 0;
}

int tmpc_ilqr_step_batch(tmpc_ctx* ctx, int B, int N, double dt, const double* x, const double* u, const double* rho,
                         int T, double* A, double* Bm, double* K, double* d, double* dV, int32_t* ok, double* alphas,
                         double* xt, double* ut, double* Jt) {
  if (!ctx) return -1;
  IlqrSweep q;
  int rc = ilqr_sweep_setup(ctx, B, N, false, q);   // what the iLQR driver refuses, its buffers and soft state
  if (rc) return rc;
  if (T != q.T)
    return fail(ctx, "tmpc_ilqr_step_batch: T = %d, but the options' alpha schedule (1, alpha_factor, ... while "
                     "alpha > alpha_min) has %d trials", T, q.T);
  if (!rho || !x || !u) return fail(ctx, "null input");
  hipSetDevice(ctx->device);
  const int nj = ctx->hmodel.n, nx = 2 * nj, Kn = N - 1;
  Work w;
  if ((rc = alloc_work(ctx, B, N, w, false))) return rc;
  ProbState st;
  if ((rc = alloc_state(ctx, B, st))) return rc;
  BUF(double, io_x, (size_t)B * nx * N);
  BUF(double, io_u, (size_t)B * nj * Kn);
  HIP_OK(hipMemcpyAsync(io_x, x, sizeof(double) * B * nx * N, hipMemcpyHostToDevice, ctx->stream));
  HIP_OK(hipMemcpyAsync(io_u, u, sizeof(double) * B * nj * Kn, hipMemcpyHostToDevice, ctx->stream));
  HIP_OK(hipMemcpyAsync(st.rho, rho, sizeof(double) * B, hipMemcpyHostToDevice, ctx->stream));
  ProbState st0 = st;   // the initial state of a solve (every problem active), but for rho: the caller's
  st0.rho = st.drho;
  launch_init_state(ctx->stream, B, 0.0, st0);
  HIP_OK(hipGetLastError());
  // xs = x[:, 0]: the trajectory is taken as given (no rollout), so the defects run_dynamics also forms are unused
  HIP_OK(hipMemcpy2DAsync(w.xs, sizeof(double), io_x, (size_t)N * sizeof(double), sizeof(double), (size_t)B * nx,
                          hipMemcpyDeviceToDevice, ctx->stream));
  if ((rc = goal_window(ctx, B, N, B, "batch size", nullptr, 0, nullptr, &w.qp.gw))) return rc;   // tmpc_set_reference
  bind_work(ctx, N, dt, io_x, io_u, st, w);
  if ((rc = ilqr_sweeps(ctx, st, w, PList{}, B, q))) return rc;
  HIP_OK(hipStreamSynchronize(ctx->stream));
  resolve_timings(ctx);
  if (A) HIP_OK(hipMemcpy(A, w.dyn.A, sizeof(double) * B * Kn * nx * nx, hipMemcpyDeviceToHost));
  if (Bm) HIP_OK(hipMemcpy(Bm, w.dyn.Bm, sizeof(double) * B * Kn * nx * nj, hipMemcpyDeviceToHost));
  if (K) HIP_OK(hipMemcpy(K, q.K, sizeof(double) * B * Kn * nj * nx, hipMemcpyDeviceToHost));
  if (d) HIP_OK(hipMemcpy(d, q.d, sizeof(double) * B * Kn * nj, hipMemcpyDeviceToHost));
  if (dV) HIP_OK(hipMemcpy(dV, q.dV, sizeof(double) * B * 2, hipMemcpyDeviceToHost));
  if (ok) HIP_OK(hipMemcpy(ok, q.ok, sizeof(int) * B, hipMemcpyDeviceToHost));
  if (alphas) HIP_OK(hipMemcpy(alphas, q.alphas, sizeof(double) * T, hipMemcpyDeviceToHost));
  if (Jt) HIP_OK(hipMemcpy(Jt, q.Jt, sizeof(double) * B * T, hipMemcpyDeviceToHost));
  // the trials are knot-major on the device ([B][T][N][nx]): the caller's are the trajectory layout [nx][N]
  if (xt) {
    std::vector<double> h((size_t)B * T * N * nx);
    HIP_OK(hipMemcpy(h.data(), q.xt, h.size() * sizeof(double), hipMemcpyDeviceToHost));
    knot_major_to_traj(B * T, N, nx, h.data(), xt);
  }
  if (ut) {
    std::vector<double> h((size_t)B * T * Kn * nj);
    HIP_OK(hipMemcpy(h.data(), q.ut, h.size() * sizeof(double), hipMemcpyDeviceToHost));
    knot_major_to_traj(B * T, Kn, nj, h.data(), ut);
  }
  return 0;
}

int tmpc_qp_blocks_batch(tmpc_ctx* ctx, int B, int N, int nx, int nu, int linsys, const double* G, const double* g,
                         const double* A, const double* Bm, const double* c, const double* rho, const double* guess,
                         double* dxul, int32_t* pcg_iters, double* S_diag, double* S_lo, double* gamma) {
  if (!ctx) return -1;
  int rc = hook_qp_sizes(ctx, "tmpc_qp_blocks_batch", B, N, nx, nu);
  if (rc) return rc;
  if (N * nx > 1024) return fail(ctx, "tmpc_qp_blocks_batch: N * nx = %d exceeds 1024 rows", N * nx);
  const int precond = precond_of(linsys);
  if (precond < 0) return fail(ctx, "linear system method %d is not available on the GPU", linsys);
  if (!G || !g || !A || !Bm || !c || !rho) return fail(ctx, "null input");
  hipSetDevice(ctx->device);
  const int K = N - 1;
  BUF(double, hb_lam, (size_t)B * N * nx);
  BUF(double, hb_Sd, (size_t)B * N * nx * nx);
  BUF(double, hb_Sl, (size_t)B * K * nx * nx);
  BUF(double, hb_gam, (size_t)B * N * nx);
  double* hb_guess = nullptr;
  if (guess && precond != 0) {
    BUF(double, hb_x0, (size_t)B * N * nx);
    HIP_OK(hipMemcpyAsync(hb_x0, guess, sizeof(double) * B * N * nx, hipMemcpyHostToDevice, ctx->stream));
    hb_guess = hb_x0;
  }
  HookQp q;
  if ((rc = hook_qp_upload(ctx, B, N, nx, nu, G, g, A, Bm, c, rho, q))) return rc;
  const double tol = ctx->opts.exit_tolerance_linSys;
  const int max_iter = ctx->opts.max_iter_linSys;
  const bool keep = S_diag || S_lo || gamma;
  QpArgs qa{};   // what every phase reads; a phase adds its mode and the outputs it writes
  qa.B = B; qa.N = N; qa.precond = PRECOND_SS; qa.G = q.Gh; qa.g = q.g; qa.A = q.A; qa.Bm = q.B; qa.cvec = q.c;
  qa.err = q.err; qa.tol = tol; qa.max_iter = max_iter; qa.iters = q.it; qa.dx = q.dx; qa.du = q.du; qa.lam = hb_lam;
  if (precond == 0) {   // methods S / N: Schur blocks -> block-Thomas -> dxu
    std::vector<int> act(B, 1);
    BUF(int, hb_act, (size_t)B);
    BUF(double, hb_U, (size_t)B * K * nx * nx);
    BUF(double, hb_Y, (size_t)B * N * nx);
    HIP_OK(hipMemcpyAsync(hb_act, act.data(), sizeof(int) * B, hipMemcpyHostToDevice, ctx->stream));
    QpArgs a = qa;
    a.mode = QP_MODE_SCHUR; a.Sd = hb_Sd; a.Sl = hb_Sl; a.gam = hb_gam;
    { Timed t(ctx, "qp_blocks_schur"); LAUNCH_OK(launch_qp_blocks(ctx->stream, nu, a)); }
    a.active = hb_act; a.U = hb_U; a.Y = hb_Y;
    { Timed t(ctx, "btsolve"); LAUNCH_OK(launch_btsolve(ctx->stream, nx, a)); }
    a = qa;
    a.mode = QP_MODE_DXU;
    { Timed t(ctx, "qp_blocks_dxu"); LAUNCH_OK(launch_qp_blocks(ctx->stream, nu, a)); }
  } else {
    QpArgs a = qa;
    a.mode = QP_MODE_PCG; a.precond = precond; a.guess = hb_guess;
    if (keep) { a.Sd = hb_Sd; a.Sl = hb_Sl; a.gam = hb_gam; }
    Timed t(ctx, "qp_blocks");
    LAUNCH_OK(launch_qp_blocks(ctx->stream, nu, a));
  }
  HIP_OK(hipStreamSynchronize(ctx->stream));
  resolve_timings(ctx);
  if ((rc = hook_qp_pivots(ctx, B, q))) return rc;
  if (dxul) {
    std::vector<double> lam((size_t)B * N * nx);
    HIP_OK(hipMemcpy(lam.data(), hb_lam, lam.size() * sizeof(double), hipMemcpyDeviceToHost));
    if ((rc = download_dxul(ctx, B, N, nx, nu, q.dx, q.du, lam.data(), dxul))) return rc;
  }
  if (pcg_iters) HIP_OK(hipMemcpy(pcg_iters, q.it, sizeof(int) * B, hipMemcpyDeviceToHost));
  if (S_diag) HIP_OK(hipMemcpy(S_diag, hb_Sd, sizeof(double) * B * N * nx * nx, hipMemcpyDeviceToHost));
  if (S_lo) HIP_OK(hipMemcpy(S_lo, hb_Sl, sizeof(double) * B * K * nx * nx, hipMemcpyDeviceToHost));
  if (gamma) HIP_OK(hipMemcpy(gamma, hb_gam, sizeof(double) * B * N * nx, hipMemcpyDeviceToHost));
  return 0;
}

int tmpc_qp_blocks_banded_batch(tmpc_ctx* ctx, int B, int N, int nx, int nu, int linsys, const double* G,
                                const double* g, const double* A, const double* Bm, const double* c,
                                const int32_t* hcnt, const int32_t* hcol, const double* hsgn, const double* hval,
                                int rmax, const double* rho, double* dxul, int32_t* pcg_iters, double* lambda_hard,
                                int32_t* singular) {
  if (!ctx) return -1;
  int rc = hook_qp_sizes(ctx, "tmpc_qp_blocks_banded_batch", B, N, nx, nu);
  if (rc) return rc;
  const int n = nx + nu, K = N - 1;
  if (rmax < 0 || rmax > 2 * n) return fail(ctx, "tmpc_qp_blocks_banded_batch: rmax = %d (0..%d)", rmax, 2 * n);
  const int precond = precond_of(linsys);
  if (precond < 0) return fail(ctx, "linear system method %d is not available on the GPU", linsys);
  if (!G || !g || !A || !Bm || !c || !rho || (rmax > 0 && (!hcnt || !hcol || !hsgn || !hval)))
    return fail(ctx, "null input");
  const int rbuf = rmax > 0 ? rmax : 1;
  std::vector<int> cnt((size_t)B * N, 0);
  if (rmax > 0) memcpy(cnt.data(), hcnt, sizeof(int) * B * N);
  for (size_t e = 0; e < cnt.size(); ++e) {
    if (cnt[e] < 0 || cnt[e] > rmax) return fail(ctx, "hard rows: %d rows at (problem, knot) %zu (0..%d)", cnt[e], e, rmax);
    for (int r = 0; r < cnt[e]; ++r) {
      const int col = hcol[e * rmax + r];
      const double sg = hsgn[e * rmax + r];
      const int k = (int)(e % N);
      if (col < 0 || col >= (k < K ? n : nx) || !(sg == 1.0 || sg == -1.0 || sg == 0.0))
        return fail(ctx, "hard row %d at (problem, knot) %zu: column %d, sign %g -- the banded QP takes box rows "
                    "(+-1 or 0 times one entry of [x_k; u_k])", r, e, col, sg);
      if (sg == 0.0 && precond != 0)
        return fail(ctx, "FULL_SET box constraints with a PCG method: the inactive rows of C are zero, so S is "
                    "singular and the reference's preconditioner raises LinAlgError (PCG.py:168-188); use method S");
    }
  }
  hipSetDevice(ctx->device);
  HookQp q;
  if ((rc = hook_qp_upload(ctx, B, N, nx, nu, G, g, A, Bm, c, rho, q))) return rc;
  BUF(int, hb_act, (size_t)B);
  HIP_OK(hipMemsetAsync(q.it, 0, sizeof(int) * B, ctx->stream));
  std::vector<int> act(B, 1);
  HIP_OK(hipMemcpyAsync(hb_act, act.data(), sizeof(int) * B, hipMemcpyHostToDevice, ctx->stream));
  HardArgs hard{};
  if ((rc = setup_hard(ctx, B, N, 0, precond, hard, nu, rmax))) return rc;
  HIP_OK(hipMemcpyAsync(hard.cnt, cnt.data(), sizeof(int) * B * N, hipMemcpyHostToDevice, ctx->stream));
  // the per-knot active-set bitmasks (tmpc_qp_hard_info), bit t * 2 nu + e of the box row over [q; qd; u]
  // and each row's slot t * 2 nu + e (the lambda_hard layout)
  std::vector<unsigned long long> amask((size_t)B * N, 0ull);
  std::vector<int> hslot((size_t)B * N * std::max(rmax, 1), 0);
  for (size_t e = 0; e < amask.size(); ++e)
    for (int r = 0; r < cnt[e]; ++r) {
      const double sg = hsgn[e * rmax + r];
      const int col = hcol[e * rmax + r], t = col / nu, i = col % nu;
      hslot[e * rmax + r] = t * 2 * nu + (sg >= 0.0 ? i : nu + i);
      if (sg != 0.0) amask[e] |= 1ull << hslot[e * rmax + r];
    }
  HIP_OK(hipMemcpyAsync(hard.amask, amask.data(), sizeof(unsigned long long) * B * N, hipMemcpyHostToDevice,
                        ctx->stream));
  if (rmax > 0)
    HIP_OK(hipMemcpyAsync(hard.hslot, hslot.data(), sizeof(int) * B * N * rmax, hipMemcpyHostToDevice, ctx->stream));
  if (rmax > 0) {
    HIP_OK(hipMemcpyAsync(hard.hcol, hcol, sizeof(int) * B * N * rbuf, hipMemcpyHostToDevice, ctx->stream));
    HIP_OK(hipMemcpyAsync(hard.hsgn, hsgn, sizeof(double) * B * N * rbuf, hipMemcpyHostToDevice, ctx->stream));
    HIP_OK(hipMemcpyAsync(hard.hval, hval, sizeof(double) * B * N * rbuf, hipMemcpyHostToDevice, ctx->stream));
  }
  hard.rows_given = 1; hard.precond = precond; hard.Ghat = q.Gh; hard.per_knot = 2; hard.gvec = q.g;
  hard.A = q.A; hard.Bm = q.B; hard.cvec = q.c; hard.jsoft = nullptr;
  hard.x = q.g; hard.u = q.g;   // not read: the gradient is the caller's (gvec), the rows are given
  hard.active = hb_act; hard.iters = q.it; hard.dx = q.dx; hard.du = q.du;
  hard.tol = ctx->opts.exit_tolerance_linSys; hard.max_iter = ctx->opts.max_iter_linSys;
  if ((rc = run_hard_qp(ctx, nu, hard))) return rc;
  HIP_OK(hipStreamSynchronize(ctx->stream));
  if ((rc = collect_hard_work(ctx, hard))) return rc;
  resolve_timings(ctx);
  if ((rc = hook_qp_pivots(ctx, B, q))) return rc;
  std::vector<int> roff((size_t)B * N), hoff((size_t)B * N);
  std::vector<double> lh((size_t)B * hard.dmax);
  HIP_OK(hipMemcpy(roff.data(), hard.roff, roff.size() * sizeof(int), hipMemcpyDeviceToHost));
  HIP_OK(hipMemcpy(hoff.data(), hard.hoff, hoff.size() * sizeof(int), hipMemcpyDeviceToHost));
  HIP_OK(hipMemcpy(lh.data(), hard.lam, lh.size() * sizeof(double), hipMemcpyDeviceToHost));
  if (dxul) {
    std::vector<double> lam((size_t)B * N * nx);
    gather_dyn_lambda(B, N, nx, hard.dmax, roff.data(), lh.data(), lam.data());
    if ((rc = download_dxul(ctx, B, N, nx, nu, q.dx, q.du, lam.data(), dxul))) return rc;
  }
  if (lambda_hard)
    for (int b = 0; b < B; ++b)
      for (int k = 0; k < N; ++k)
        for (int r = 0; r < rbuf; ++r)
          lambda_hard[((size_t)b * N + k) * rbuf + r] =
              r < cnt[(size_t)b * N + k] ? lh[(size_t)b * hard.dmax + hoff[(size_t)b * N + k] + r] : 0.0;
  if (pcg_iters) HIP_OK(hipMemcpy(pcg_iters, q.it, sizeof(int) * B, hipMemcpyDeviceToHost));
  if (singular) HIP_OK(hipMemcpy(singular, hard.sing, sizeof(int) * B, hipMemcpyDeviceToHost));
  ctx->hard_last = {B, N, hard.dmax, hard.W, hard.rmax};   // tmpc_qp_hard_info reads this QP's S band and gamma
  return 0;
}

int tmpc_qp_hard_info(tmpc_ctx* ctx, int B, int N, int32_t* sizes, int32_t* dim, uint64_t* active,
                      double* lambda_hard, double* S_band, double* gamma, int32_t* singular) {
  if (!ctx) return -1;
  const auto& hl = ctx->hard_last;
  if (hl.B == 0)
    return fail(ctx, "tmpc_qp_hard_info: the last tmpc_qp_batch did not take the banded path (hard box limits, or "
                "N * nx past %d rows)", QP_MAX_ROWS);
  if (hl.B != B || hl.N != N)
    return fail(ctx, "tmpc_qp_hard_info: the last hard-limit QP was B=%d N=%d, asked for B=%d N=%d", hl.B, hl.N, B, N);
  hipSetDevice(ctx->device);
  const int nj = ctx->hmodel.n, S6 = 6 * nj;
  if (sizes) {
    sizes[0] = hl.dmax;
    sizes[1] = hl.W;
  }
  const HardArgs& hd = ctx->hard_dev;   // that QP's buffers (setup_hard)
  if (dim) HIP_OK(hipMemcpy(dim, hd.dim, sizeof(int) * B, hipMemcpyDeviceToHost));
  if (active) HIP_OK(hipMemcpy(active, hd.amask, sizeof(uint64_t) * B * N, hipMemcpyDeviceToHost));
  if (singular) HIP_OK(hipMemcpy(singular, hd.sing, sizeof(int) * B, hipMemcpyDeviceToHost));
  const size_t BW = 2 * (size_t)hl.W + 1;
  if (S_band) {
    // the device band is written only inside each row's structural range (k_hard_schur); the ABI's is zero
    // outside the ranges (tmpc_host_pack.h)
    std::vector<double> sbt((size_t)B * hl.dmax * BW);
    HIP_OK(hipMemcpy(sbt.data(), hd.Sb, sizeof(double) * sbt.size(), hipMemcpyDeviceToHost));
    std::vector<int> rg((size_t)B * hl.dmax * 2), dm(B);
    HIP_OK(hipMemcpy(rg.data(), hd.rng, rg.size() * sizeof(int), hipMemcpyDeviceToHost));
    HIP_OK(hipMemcpy(dm.data(), hd.dim, B * sizeof(int), hipMemcpyDeviceToHost));
    band_dev_to_abi(B, hl.dmax, hl.W, dm.data(), rg.data(), sbt.data(), S_band);
  }
  if (gamma) HIP_OK(hipMemcpy(gamma, hd.gam, sizeof(double) * B * hl.dmax, hipMemcpyDeviceToHost));
  if (lambda_hard) {
    // the hard rows' multipliers by slot t * 2n + e (0 where the slot has no row); rmax as hd_slot was laid out
    const int rmax = hl.rmax;
    std::vector<int> cnt((size_t)B * N), hoff((size_t)B * N), slot((size_t)B * N * rmax);
    std::vector<double> lam((size_t)B * hl.dmax);
    HIP_OK(hipMemcpy(cnt.data(), hd.cnt, cnt.size() * sizeof(int), hipMemcpyDeviceToHost));
    HIP_OK(hipMemcpy(hoff.data(), hd.hoff, hoff.size() * sizeof(int), hipMemcpyDeviceToHost));
    HIP_OK(hipMemcpy(slot.data(), hd.hslot, slot.size() * sizeof(int), hipMemcpyDeviceToHost));
    HIP_OK(hipMemcpy(lam.data(), hd.lam, lam.size() * sizeof(double), hipMemcpyDeviceToHost));
    memset(lambda_hard, 0, sizeof(double) * B * N * S6);
    for (int b = 0; b < B; ++b)
      for (int k = 0; k < N; ++k) {
        const size_t bk = (size_t)b * N + k;
        for (int r = 0; r < cnt[bk] && r < rmax; ++r) {
          const int sl = slot[bk * rmax + r];
          if (sl >= 0 && sl < S6) lambda_hard[bk * S6 + sl] = lam[(size_t)b * hl.dmax + hoff[bk] + r];
        }
      }
  }
  return 0;
}

int tmpc_hard_pcg_batch(tmpc_ctx* ctx, int B, int nx, int dmax, int W, const int32_t* dim, int precond,
                        const double* S_band, const double* gamma, double tol, int max_iter, double* lambda,
                        int32_t* iters) {
  if (!ctx) return -1;
  if (B < 1 || nx < 2 || nx > 14 || (nx & 1) || dmax < 1 || W < 0 || W > 1024)
    return fail(ctx, "bad sizes B=%d nx=%d dmax=%d W=%d", B, nx, dmax, W);
  if (int rc = pcg_precond_ok(ctx, precond)) return rc;
  if (dmax > HARD_PCG_MAX_ROWS) return fail(ctx, "dmax = %d exceeds the PCG's %d rows", dmax, HARD_PCG_MAX_ROWS);
  if (max_iter < 0) return fail(ctx, "max_iter must be >= 0");
  if (!dim || !S_band || !gamma) return fail(ctx, "null input");
  for (int b = 0; b < B; ++b)
    if (dim[b] < 1 || dim[b] > dmax) return fail(ctx, "dim[%d] = %d outside [1, %d]", b, dim[b], dmax);
  hipSetDevice(ctx->device);
  const size_t BW = 2 * (size_t)W + 1, nbmax = dmax / nx + 1;
  BUF(double, hp_Sb, (size_t)B * dmax * BW);
  BUF(double, hp_gam, (size_t)B * dmax);
  BUF(double, hp_lam, (size_t)B * dmax);
  BUF(int, hp_dim, (size_t)B);
  BUF(int, hp_act, (size_t)B);
  BUF(int, hp_it, (size_t)B);
  BUF(double, hp_Pd, (size_t)B * nbmax * nx * nx);
  BUF(double, hp_Pl, (size_t)B * nbmax * nx * nx);
  BUF(double, hp_Ptr, (size_t)B * nbmax * nx * nx);
  BUF(int, hp_rng, (size_t)B * dmax * 2);
  // the ABI's row-major band to the device's row-start-relative one and each row's first / last nonzero
  // column, the range the kernel's products visit (tmpc_host_pack.h)
  std::vector<int> rg((size_t)B * dmax * 2);
  std::vector<double> sbt((size_t)B * dmax * BW);
  band_abi_to_dev(B, dmax, W, dim, S_band, rg.data(), sbt.data());
  HIP_OK(hipMemcpyAsync(hp_rng, rg.data(), rg.size() * sizeof(int), hipMemcpyHostToDevice, ctx->stream));
  HIP_OK(hipMemcpy(hp_Sb, sbt.data(), sizeof(double) * B * dmax * BW, hipMemcpyHostToDevice));
  HIP_OK(hipMemcpyAsync(hp_gam, gamma, sizeof(double) * B * dmax, hipMemcpyHostToDevice, ctx->stream));
  HIP_OK(hipMemcpyAsync(hp_dim, dim, sizeof(int) * B, hipMemcpyHostToDevice, ctx->stream));
  std::vector<int> ones(B, 1);
  HIP_OK(hipMemcpyAsync(hp_act, ones.data(), sizeof(int) * B, hipMemcpyHostToDevice, ctx->stream));
  HardArgs h{};
  h.B = B; h.precond = precond; h.dmax = dmax; h.W = W; h.tol = tol; h.max_iter = max_iter;
  h.active = hp_act; h.dim = hp_dim; h.Sb = hp_Sb; h.gam = hp_gam; h.Pd = hp_Pd; h.Pl = hp_Pl; h.Ptr = hp_Ptr;
  h.lam = hp_lam; h.iters = hp_it; h.rng = hp_rng;
  int rc;
  BUF(double, hp_work, (size_t)B);
  HIP_OK(hipMemsetAsync(hp_work, 0, sizeof(double) * B, ctx->stream));
  h.work = hp_work;
  {
    Timed t(ctx, "hard_pcg");
    LAUNCH_OK(launch_hard_solve(ctx->stream, nx / 2, h));
  }
  if ((rc = collect_hard_work(ctx, h))) return rc;
  resolve_timings(ctx);
  if (lambda) HIP_OK(hipMemcpy(lambda, hp_lam, sizeof(double) * B * dmax, hipMemcpyDeviceToHost));
  if (iters) HIP_OK(hipMemcpy(iters, hp_it, sizeof(int) * B, hipMemcpyDeviceToHost));
  return 0;
}

int tmpc_pcg_batch(tmpc_ctx* ctx, int B, int N, int nx, int precond, const double* S_diag, const double* S_lo,
                   const double* S_up, const double* gamma, const double* guess, double tol, int max_iter,
                   double* lambda,
                   int32_t* iters, double* trace_nu, double* trace_res, double* P_diag) {
  if (!ctx) return -1;
  if (B < 1 || N < 1 || nx < 1) return fail(ctx, "bad sizes B=%d N=%d nx=%d", B, N, nx);
  if (N * nx > 1024) return fail(ctx, "N * nx = %d exceeds 1024 rows", N * nx);
  if (int rc = pcg_precond_ok(ctx, precond)) return rc;
  if (max_iter < 0) return fail(ctx, "max_iter must be >= 0");
  if (!S_diag || !gamma || (N > 1 && !S_lo)) return fail(ctx, "null input");
  hipSetDevice(ctx->device);
  const int K = N - 1;
  BUF(double, p_Sd, (size_t)B * N * nx * nx);
  BUF(double, p_Sl, (size_t)B * (K > 0 ? K : 1) * nx * nx);
  BUF(double, p_Su, (size_t)B * (K > 0 ? K : 1) * nx * nx);
  BUF(double, p_g, (size_t)B * N * nx);
  BUF(double, p_lam, (size_t)B * N * nx);
  BUF(int, p_it, (size_t)B);
  BUF(double, p_tn, (size_t)B * (max_iter + 1));
  BUF(double, p_tr, (size_t)B * (max_iter + 1));
  BUF(double, p_Pd, (size_t)B * N * nx * nx);
  BUF(double, p_x0, (size_t)B * N * nx);
  if (guess) HIP_OK(hipMemcpyAsync(p_x0, guess, sizeof(double) * B * N * nx, hipMemcpyHostToDevice, ctx->stream));
  HIP_OK(hipMemcpyAsync(p_Sd, S_diag, sizeof(double) * B * N * nx * nx, hipMemcpyHostToDevice, ctx->stream));
  if (K > 0) HIP_OK(hipMemcpyAsync(p_Sl, S_lo, sizeof(double) * B * K * nx * nx, hipMemcpyHostToDevice, ctx->stream));
  if (K > 0 && S_up)
    HIP_OK(hipMemcpyAsync(p_Su, S_up, sizeof(double) * B * K * nx * nx, hipMemcpyHostToDevice, ctx->stream));
  HIP_OK(hipMemcpyAsync(p_g, gamma, sizeof(double) * B * N * nx, hipMemcpyHostToDevice, ctx->stream));
  {
    QpArgs a{};   // the optional inputs and outputs the caller gave
    a.B = B; a.N = N; a.precond = precond; a.Sd = p_Sd; a.Sl = p_Sl; a.gam = p_g; a.tol = tol; a.max_iter = max_iter;
    a.lam = p_lam; a.iters = p_it;
    a.Su = S_up ? p_Su : nullptr; a.guess = guess ? p_x0 : nullptr; a.Pd = P_diag ? p_Pd : nullptr;
    a.tnu = trace_nu ? p_tn : nullptr; a.tres = trace_res ? p_tr : nullptr;
    Timed t(ctx, "pcg");
    LAUNCH_OK(launch_pcg(ctx->stream, nx, a));
  }
  HIP_OK(hipStreamSynchronize(ctx->stream));
  resolve_timings(ctx);
  if (lambda) HIP_OK(hipMemcpy(lambda, p_lam, sizeof(double) * B * N * nx, hipMemcpyDeviceToHost));
  if (iters) HIP_OK(hipMemcpy(iters, p_it, sizeof(int) * B, hipMemcpyDeviceToHost));
  if (trace_nu) HIP_OK(hipMemcpy(trace_nu, p_tn, sizeof(double) * B * (max_iter + 1), hipMemcpyDeviceToHost));
  if (trace_res) HIP_OK(hipMemcpy(trace_res, p_tr, sizeof(double) * B * (max_iter + 1), hipMemcpyDeviceToHost));
  if (P_diag && precond != PRECOND_J)
    HIP_OK(hipMemcpy(P_diag, p_Pd, sizeof(double) * B * N * nx * nx, hipMemcpyDeviceToHost));
  return 0;
}

int tmpc_pcg_dense_batch(tmpc_ctx* ctx, int B, int D, const double* A, const double* b, const double* Pinv,
                         int precond, int nx, const double* guess, double tol, int max_iter, double* x,
                         int32_t* iters, double* trace_nu, double* trace_res, double* Pinv_out) {
  if (!ctx) return -1;
  if (B < 1 || D < 1 || (size_t)B * D * D > ((size_t)1 << 34))
    return fail(ctx, "bad sizes B=%d D=%d (the dense PCG takes D >= 1 and B D^2 <= 2^34 entries)", B, D);
  if (!A || !b) return fail(ctx, "null input");
  if (max_iter < 0) return fail(ctx, "max_iter must be >= 0");
  if (!Pinv) {
    if (int rc = pcg_precond_ok(ctx, precond)) return rc;
    if ((precond == PRECOND_BJ || precond == PRECOND_SS) && (nx < 1 || nx > 16))
      return fail(ctx, "block size %d: the device preconditioner takes 1..16", nx);
  }
  hipSetDevice(ctx->device);
  const size_t DD = (size_t)B * D * D;
  BUF(double, dn_stage, DD);
  BUF(double, dn_AT, DD);
  BUF(double, dn_PT, DD);
  BUF(double, dn_b, (size_t)B * D);
  BUF(double, dn_x0, (size_t)B * D);
  BUF(double, dn_x, (size_t)B * D);
  BUF(int, dn_it, (size_t)B);
  BUF(double, dn_tn, (size_t)B * (max_iter + 1));
  BUF(double, dn_tr, (size_t)B * (max_iter + 1));
  const int nbk = (!Pinv && (precond == PRECOND_BJ || precond == PRECOND_SS)) ? D / nx : 0;
  BUF(double, dn_Pd, (size_t)B * (nbk + 1) * (nx > 0 ? nx * nx : 1));
  DenseArgs a{};
  a.B = B; a.D = D; a.nx = nx; a.precond = precond; a.max_iter = max_iter; a.tol = tol; a.A = dn_stage;
  a.b = dn_b; a.guess = guess ? dn_x0 : nullptr; a.AT = dn_AT; a.PT = dn_PT; a.Pd = dn_Pd; a.x = dn_x;
  a.iters = dn_it; a.trace_nu = trace_nu ? dn_tn : nullptr; a.trace_res = trace_res ? dn_tr : nullptr;
  const bool big = D > HARD_PCG_MAX_ROWS;   // past the one-workgroup kernel's registers / LDS
  if (big) {
    BUF(double, dn_r, (size_t)B * D);
    BUF(double, dn_p, (size_t)B * D);
    BUF(double, dn_y, (size_t)B * D);
    BUF(double, dn_q, (size_t)B * D);
    BUF(double, dn_nu, (size_t)B);
    BUF(int, dn_done, (size_t)B);
    a.r = dn_r; a.p = dn_p; a.y = dn_y; a.q = dn_q; a.nu = dn_nu; a.done = dn_done;
  }
  HIP_OK(hipMemcpyAsync(dn_stage, A, sizeof(double) * DD, hipMemcpyHostToDevice, ctx->stream));
  HIP_OK(hipMemcpyAsync(dn_b, b, sizeof(double) * B * D, hipMemcpyHostToDevice, ctx->stream));
  if (guess) HIP_OK(hipMemcpyAsync(dn_x0, guess, sizeof(double) * B * D, hipMemcpyHostToDevice, ctx->stream));
  {
    Timed t(ctx, "pcg_dense");
    LAUNCH_OK(launch_dense_transpose(ctx->stream, B, D, dn_stage, dn_AT));
    if (Pinv) {
      HIP_OK(hipMemcpyAsync(dn_stage, Pinv, sizeof(double) * DD, hipMemcpyHostToDevice, ctx->stream));
      LAUNCH_OK(launch_dense_transpose(ctx->stream, B, D, dn_stage, dn_PT));
    } else {
      HIP_OK(hipMemsetAsync(dn_PT, 0, sizeof(double) * DD, ctx->stream));
      LAUNCH_OK(launch_dense_precond(ctx->stream, a));   // reads A row-major from the stage
    }
    if (big) LAUNCH_OK(launch_pcg_dense_big(ctx->stream, a));
    else LAUNCH_OK(launch_pcg_dense(ctx->stream, a));
  }
  HIP_OK(hipStreamSynchronize(ctx->stream));
  resolve_timings(ctx);
  if (x) HIP_OK(hipMemcpy(x, dn_x, sizeof(double) * B * D, hipMemcpyDeviceToHost));
  if (iters) HIP_OK(hipMemcpy(iters, dn_it, sizeof(int) * B, hipMemcpyDeviceToHost));
  if (trace_nu) HIP_OK(hipMemcpy(trace_nu, dn_tn, sizeof(double) * B * (max_iter + 1), hipMemcpyDeviceToHost));
  if (trace_res) HIP_OK(hipMemcpy(trace_res, dn_tr, sizeof(double) * B * (max_iter + 1), hipMemcpyDeviceToHost));
  if (Pinv_out) {   // Pinv = PT^T: back through the transpose, into the stage
    LAUNCH_OK(launch_dense_transpose(ctx->stream, B, D, dn_PT, dn_stage));
    HIP_OK(hipMemcpyAsync(Pinv_out, dn_stage, sizeof(double) * DD, hipMemcpyDeviceToHost, ctx->stream));
    HIP_OK(hipStreamSynchronize(ctx->stream));
  }
  return 0;
}

}  // extern "C"
