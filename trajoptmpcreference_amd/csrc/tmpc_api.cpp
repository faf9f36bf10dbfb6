// C ABI (include/tmpc.h): the context, its configuration, the batch / stream / MPC solve entry points and the
// memory and statistics accessors.  The solver drivers are in tmpc_solve.cpp, the unit entry points in
// tmpc_api_qp.cpp.
#include <hip/hip_runtime.h>

#include <cstdlib>
#include <cstring>
#include <string>

#include "tmpc_ctx.h"

using namespace tmpc;

namespace {

// exit code and iteration count per problem of the last solve
int read_status(tmpc_ctx* ctx, int B, int32_t* exit_code, int32_t* iters) {
  if (exit_code) HIP_OK(hipMemcpy(exit_code, ctx->last_st.exit_sqp, sizeof(int) * B, hipMemcpyDeviceToHost));
  if (iters) HIP_OK(hipMemcpy(iters, ctx->last_st.iter, sizeof(int) * B, hipMemcpyDeviceToHost));
  return 0;
}

// the trace rows [B][max_iter_SQP_DDP + 1] the caller asked for; hard_active only when the solve recorded it
int copy_trace(tmpc_ctx* ctx, int B, int N, const TraceDev& tr, bool hard_trace, tmpc_trace* trace) {
  const size_t n = (size_t)B * (ctx->opts.max_iter_SQP_DDP + 1);
  const struct { void* dst; const void* src; size_t elem; } rows[] = {
      {trace->iteration, tr.iteration, sizeof(int)},
      {trace->line_search_iteration, tr.ls_iter, sizeof(int)},
      {trace->alpha, tr.alpha, sizeof(double)},
      {trace->rho, tr.rho, sizeof(double)},
      {trace->J, tr.J, sizeof(double)},
      {trace->c, tr.c, sizeof(double)},
      {trace->merit, tr.merit, sizeof(double)},
      {trace->D, tr.D, sizeof(double)},
      {trace->reduction_ratio, tr.ratio, sizeof(double)},
      {trace->succeeded_line_search, tr.accepted, sizeof(int)},
      {trace->pcg_iters, tr.pcg_iters, sizeof(int)},
      {trace->singular, tr.singular, sizeof(int)},
  };
  for (const auto& r : rows)
    if (r.dst) HIP_OK(hipMemcpy(r.dst, r.src, n * r.elem, hipMemcpyDeviceToHost));
  if (trace->hard_active) {
    if (hard_trace)
      HIP_OK(hipMemcpy(trace->hard_active, tr.hard_active, n * N * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    else
      memset(trace->hard_active, 0, n * N * sizeof(uint64_t));
  }
  return 0;
}

// A batch solve on host arrays: x, u up, driver(d_x, d_u, &trace buffers), x, u, the status arrays and the
// trace down.  qp: the SQP's size limits (check_ready).
template <class Driver>
int solve_host(tmpc_ctx* ctx, int B, int N, bool qp, double* x, double* u, int32_t* exit_code, int32_t* exit_soft,
               int32_t* outer_iter, int32_t* iters, tmpc_trace* trace, bool hard_trace, Driver driver) {
  int rc = check_ready(ctx, B, N, qp);
  if (rc) return rc;
  if (!x || !u) return fail(ctx, "null x/u");
  hipSetDevice(ctx->device);
  const int nx = ctx->hcost.nx, nu = ctx->hcost.nu;
  const size_t xn = (size_t)B * nx * N, un = (size_t)B * nu * (N - 1);
  BUF(double, io_x, xn);
  BUF(double, io_u, un);
  HIP_OK(hipMemcpyAsync(io_x, x, xn * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
  HIP_OK(hipMemcpyAsync(io_u, u, un * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
  TraceDev tr;
  if ((rc = driver(io_x, io_u, &tr))) return rc;
  HIP_OK(hipMemcpy(x, io_x, xn * sizeof(double), hipMemcpyDeviceToHost));
  HIP_OK(hipMemcpy(u, io_u, un * sizeof(double), hipMemcpyDeviceToHost));
  if ((rc = read_status(ctx, B, exit_code, iters))) return rc;
  if (exit_soft) HIP_OK(hipMemcpy(exit_soft, ctx->exit_soft, sizeof(int) * B, hipMemcpyDeviceToHost));
  if (outer_iter) HIP_OK(hipMemcpy(outer_iter, ctx->outer_iter, sizeof(int) * B, hipMemcpyDeviceToHost));
  return trace ? copy_trace(ctx, B, N, tr, hard_trace, trace) : 0;
}

// the quadratic part of either cost
CostDev quadratic_terms(int nx, int nu, const double* Q, const double* QF, const double* R, const double* xg,
                        int32_t QF_start) {
  CostDev c{};
  c.nx = nx;
  c.nu = nu;
  c.QF_start = QF_start < 0 ? -1 : QF_start;
  memcpy(c.Q, Q, sizeof(double) * nx * nx);
  memcpy(c.QF, QF, sizeof(double) * nx * nx);
  memcpy(c.R, R, sizeof(double) * nu * nu);
  memcpy(c.xg, xg, sizeof(double) * nx);
  return c;
}

int set_cost(tmpc_ctx* ctx, const CostDev& c) {
  hipSetDevice(ctx->device);
  HIP_OK(hipMemcpyAsync(ctx->dcost, &c, sizeof(c), hipMemcpyHostToDevice, ctx->stream));
  HIP_OK(hipStreamSynchronize(ctx->stream));
  ctx->hcost = c;
  ctx->has_cost = true;
  ctx->mpc_last.B = 0;   // (QF_start counts down along an MPC step loop)
  return 0;
}

int copy_sync(tmpc_ctx* ctx, void* dst, const void* src, size_t bytes, hipMemcpyKind kind) {
  if (!ctx) return -1;
  hipSetDevice(ctx->device);
  HIP_OK(hipMemcpyAsync(dst, src, bytes, kind, ctx->stream));
  HIP_OK(hipStreamSynchronize(ctx->stream));
  return 0;
}

}  // namespace

// ======================================================================= C ABI
extern "C" {

int tmpc_abi_version(void) { return TMPC_ABI_VERSION; }

int tmpc_device_count(int* count) {
  if (!count) return -1;
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) n = 0;
  *count = n;
  return 0;
}

int tmpc_create(int device, tmpc_ctx** out) {
  if (!out) return -1;
  *out = nullptr;
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess || n == 0) return -2;
  if (device < 0 || device >= n) return -3;
  tmpc_ctx* ctx = new tmpc_ctx();
  ctx->device = device;
  if (hipSetDevice(device) != hipSuccess || hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking) != hipSuccess ||
      hipMalloc(&ctx->dmodel, sizeof(ModelDev)) != hipSuccess || hipMalloc(&ctx->dcost, sizeof(CostDev)) != hipSuccess ||
      hipMalloc(&ctx->dlim, sizeof(ConstrDev)) != hipSuccess || hipMemset(ctx->dlim, 0, sizeof(ConstrDev)) != hipSuccess ||
      hipHostMalloc(&ctx->h_count, 8 * sizeof(int)) != hipSuccess) {
    delete ctx;
    return -4;
  }
  pcg_set_max_lds();
  hard_set_max_lds();
  dense_set_max_lds();
  qp_blocks_set_max_lds();
  tmpc_default_options(&ctx->opts);
  *out = ctx;
  return 0;
}

void tmpc_destroy(tmpc_ctx* ctx) {
  if (!ctx) return;
  hipSetDevice(ctx->device);
  if (ctx->stream) hipStreamSynchronize(ctx->stream);
  for (auto& p : ctx->pending) {
    hipEventDestroy(p.start);
    hipEventDestroy(p.stop);
  }
  for (auto e : ctx->event_pool) hipEventDestroy(e);
  for (tmpc_ctx* sub : ctx->subs) tmpc_destroy(sub);
  for (auto& kv : ctx->bufs)
    if (kv.second.ptr) hipFree(kv.second.ptr);
  if (ctx->dmodel) hipFree(ctx->dmodel);
  if (ctx->dcost) hipFree(ctx->dcost);
  if (ctx->dlim) hipFree(ctx->dlim);
  if (ctx->h_count) hipHostFree(ctx->h_count);
  if (ctx->stream) hipStreamDestroy(ctx->stream);
  delete ctx;
}

const char* tmpc_last_error(const tmpc_ctx* ctx) { return ctx ? ctx->err.c_str() : "null context"; }

int tmpc_set_model(tmpc_ctx* ctx, int n, const int32_t* parent, const int32_t* jtype, const int32_t* saxis,
                   const double* X0, const double* Xa, const double* Xb, const double* I, double gravity) {
  if (!ctx) return -1;
  if (n < 1 || n > NJMAX) return fail(ctx, "model must have 1..%d joints (got %d)", NJMAX, n);
  if (!parent || !jtype || !saxis || !X0 || !Xa || !Xb || !I) return fail(ctx, "null model array");
  ModelDev m{};
  m.n = n;
  m.gravity = gravity;
  bool chain = true;
  for (int j = 0; j < n; ++j) {
    if (parent[j] < -1 || parent[j] >= j)
      return fail(ctx, "parent[%d] = %d: joints must be in DFS order (parent id < child id)", j, parent[j]);
    if (jtype[j] != TMPC_JOINT_REVOLUTE && jtype[j] != TMPC_JOINT_PRISMATIC)
      return fail(ctx, "joint %d: unsupported joint type %d", j, jtype[j]);
    if (saxis[j] < 0 || saxis[j] > 5) return fail(ctx, "joint %d: motion subspace index %d out of range", j, saxis[j]);
    m.parent[j] = parent[j];
    m.jtype[j] = jtype[j];
    m.saxis[j] = saxis[j];
    if (parent[j] != j - 1) chain = false;
    for (int e = 0; e < 6; ++e) m.S[j][e] = (e == saxis[j]) ? 1.0 : 0.0;
    memcpy(m.X0[j], X0 + 36 * j, 36 * sizeof(double));
    memcpy(m.Xa[j], Xa + 36 * j, 36 * sizeof(double));
    memcpy(m.Xb[j], Xb + 36 * j, 36 * sizeof(double));
    memcpy(m.I[j], I + 36 * j, 36 * sizeof(double));
  }
  for (int j = n - 1; j >= 0; --j) {
    m.subtree[j] |= 1u << j;
    if (parent[j] >= 0) m.subtree[parent[j]] |= m.subtree[j];
  }
  m.chain = chain ? 1 : 0;
  // per-robot compiled kernels when the model is one of the bundled ones (tools/gen_models.py);
  // TMPC_GENERIC_MODEL=1 forces the runtime-coefficient kernels
  const char* gen = getenv("TMPC_GENERIC_MODEL");
  ctx->model_id = (gen && gen[0] == '1') ? 0 : match_static_model(m);
  ctx->soft_B = ctx->soft_N = -1;   // the soft-constraint state is sized per model (6 n slots per knot)
  ctx->mpc_last.B = 0;
  ctx->ref_dev = nullptr;           // and so is a state reference (nx rows)
  ctx->ref_R = ctx->ref_M = 0;
  hipSetDevice(ctx->device);
  HIP_OK(hipMemcpyAsync(ctx->dmodel, &m, sizeof(m), hipMemcpyHostToDevice, ctx->stream));
  HIP_OK(hipStreamSynchronize(ctx->stream));
  ctx->hmodel = m;
  ctx->has_model = true;
  return 0;
}

int tmpc_set_cost_quadratic(tmpc_ctx* ctx, int nx, int nu, const double* Q, const double* QF, const double* R,
                            const double* xg, int32_t QF_start) {
  if (!ctx) return -1;
  if (nx < 1 || nx > NXMAX || nu < 1 || nu > NJMAX) return fail(ctx, "cost sizes out of range (nx=%d, nu=%d)", nx, nu);
  if (!Q || !QF || !R || !xg) return fail(ctx, "null cost array");
  CostDev c = quadratic_terms(nx, nu, Q, QF, R, xg, QF_start);
  // diagonal Q, QF, R: the kernels' cost products take their exact-zero-free form (CostDev.diag);
  // TMPC_GENERIC_COST=1 keeps the dense form (tests compare the two bit for bit)
  const char* gc = getenv("TMPC_GENERIC_COST");
  c.diag = (gc && gc[0] == '1') ? 0 : 1;
  for (int r = 0; r < nx; ++r)
    for (int k = 0; k < nx; ++k)
      if (r != k && (Q[r * nx + k] != 0.0 || QF[r * nx + k] != 0.0)) c.diag = 0;
  for (int r = 0; r < nu; ++r)
    for (int k = 0; k < nu; ++k)
      if (r != k && R[r * nu + k] != 0.0) c.diag = 0;
  return set_cost(ctx, c);
}

int tmpc_set_cost_ee(tmpc_ctx* ctx, int nx, int nu, const double* Q, const double* QF, const double* R,
                     const double* xg, int32_t QF_start, const double* H0, const double* Ha, const double* Hb) {
  if (!ctx) return -1;
  if (nx != 4 || nu != 2)
    return fail(ctx, "UrdfCost is defined for 2-link arms only (nx=4, nu=2; got nx=%d, nu=%d)", nx, nu);
  if (!Q || !QF || !R || !xg || !H0 || !Ha || !Hb) return fail(ctx, "null cost array");
  CostDev c = quadratic_terms(nx, nu, Q, QF, R, xg, QF_start);
  c.kind = COST_EE;
  memcpy(c.eeH0, H0, sizeof(double) * 32);
  memcpy(c.eeHa, Ha, sizeof(double) * 32);
  memcpy(c.eeHb, Hb, sizeof(double) * 32);
  return set_cost(ctx, c);
}

// The state reference xref [R][nx][M] (include/tmpc.h): copied into the context's own buffer, host or device source.
static int set_reference(tmpc_ctx* ctx, int R, int M, const double* xref, hipMemcpyKind kind) {
  if (!ctx) return -1;
  if (R == 0 || !xref) {   // clear: every kernel reads the cost's xg again
    ctx->ref_dev = nullptr;
    ctx->ref_R = ctx->ref_M = 0;
    return 0;
  }
  if (!ctx->has_model) return fail(ctx, "no model: call tmpc_set_model first (a reference has nx = 2 n rows)");
  if (R < 1 || M < 1) return fail(ctx, "reference sizes R = %d, M = %d (both >= 1; R = 0 clears)", R, M);
  hipSetDevice(ctx->device);
  const size_t count = (size_t)R * 2 * ctx->hmodel.n * M;
  BUF(double, ref_xref, count);
  HIP_OK(hipMemcpyAsync(ref_xref, xref, count * sizeof(double), kind, ctx->stream));
  HIP_OK(hipStreamSynchronize(ctx->stream));
  ctx->ref_dev = ref_xref;
  ctx->ref_R = R;
  ctx->ref_M = M;
  return 0;
}

int tmpc_set_reference(tmpc_ctx* ctx, int R, int M, const double* xref) {
  return set_reference(ctx, R, M, xref, hipMemcpyHostToDevice);
}

int tmpc_set_reference_device(tmpc_ctx* ctx, int R, int M, const double* d_xref) {
  return set_reference(ctx, R, M, d_xref, hipMemcpyDeviceToDevice);
}

void tmpc_default_options(tmpc_options* o) {
  if (!o) return;
  memset(o, 0, sizeof(*o));
  o->exit_tolerance_linSys = 1e-6;
  o->max_iter_linSys = 100;
  o->max_iter_SQP_DDP = 100;
  o->exit_tolerance_SQP_DDP = 1e-6;
  o->alpha_factor_SQP_DDP = 0.5;
  o->alpha_min_SQP_DDP = 0.005;
  o->rho_factor_SQP_DDP = 4;
  o->rho_min_SQP_DDP = 1e-3;
  o->rho_max_SQP_DDP = 1e3;
  o->rho_init_SQP_DDP = 0.001;
  o->expected_reduction_min_SQP_DDP = 0.05;
  o->expected_reduction_max_SQP_DDP = 3;
  o->merit_mu = 10.0;
  o->profile = 0;
  o->max_iter_softConstraints = 10;
  o->exit_tolerance_softConstraints = 1e-6;
}

int tmpc_set_box_limits(tmpc_ctx* ctx, const tmpc_box_limits* L) {
  if (!ctx) return -1;
  if (!ctx->has_model) return fail(ctx, "no model: call tmpc_set_model first");
  ctx->hard_last = {0, 0, 0, 0, 0};
  ConstrDev c{};
  if (L) {
    for (int t = 0; t < 3; ++t) {
      if (L->mode[t] < TMPC_LIMIT_NONE || L->mode[t] > TMPC_LIMIT_FULL_SET)
        return fail(ctx, "limit %d: mode %d (valid: 0 none, 1 QUADRATIC_PENALTY, 2 AUGMENTED_LAGRANGIAN, "
                    "3 ACTIVE_SET, 4 FULL_SET)", t, L->mode[t]);
      if (L->mode[t] <= TMPC_LIMIT_AUGMENTED_LAGRANGIAN) {
        c.mode[t] = L->mode[t];
        if (c.mode[t] != SOFT_NONE) c.any = 1;
      } else {
        c.hard[t] = L->mode[t] == TMPC_LIMIT_ACTIVE_SET ? HARD_ACTIVE : HARD_FULL;
        c.any_hard = 1;
      }
      constexpr int abi_row = (int)(sizeof(L->lb[0]) / sizeof(double));   // tmpc_box_limits rows: 8 joints
      for (int i = 0; i < NJMAX; ++i) {   // (limits are refused past NJ_FULL joints, check_ready)
        c.lb[t][i] = i < abi_row ? L->lb[t][i] : 0.0;
        c.ub[t][i] = i < abi_row ? L->ub[t][i] : 0.0;
      }
      c.mu_init[t] = L->mu_init[t];
      c.mu_factor[t] = L->mu_factor[t];
      c.mu_max[t] = L->mu_max[t];
      c.phi_init[t] = L->phi_init[t];
      c.phi_factor[t] = L->phi_factor[t];
    }
  }
  hipSetDevice(ctx->device);
  HIP_OK(hipMemcpyAsync(ctx->dlim, &c, sizeof(c), hipMemcpyHostToDevice, ctx->stream));
  HIP_OK(hipStreamSynchronize(ctx->stream));
  ctx->hlim = c;
  ctx->soft_B = ctx->soft_N = -1;
  ctx->mpc_last.B = 0;
  return 0;
}

int tmpc_set_soft_state(tmpc_ctx* ctx, int B, int N, const double* mu, const double* lam, const double* phi) {
  if (!ctx) return -1;
  if (!ctx->has_model) return fail(ctx, "no model: call tmpc_set_model first");
  if (B < 1 || N < 2) return fail(ctx, "bad sizes B=%d N=%d", B, N);
  hipSetDevice(ctx->device);
  int rc = alloc_soft(ctx, B, N);
  if (rc) return rc;
  double *smu = ctx->soft_mu, *slam = ctx->soft_lam, *sphi = ctx->soft_phi;
  const size_t n = (size_t)B * N * 6 * ctx->hmodel.n;
  launch_soft_init(ctx->stream, ctx->dlim, n, 6 * ctx->hmodel.n, smu, slam, sphi);
  HIP_OK(hipGetLastError());
  if (mu) HIP_OK(hipMemcpyAsync(smu, mu, n * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
  if (lam) HIP_OK(hipMemcpyAsync(slam, lam, n * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
  if (phi) HIP_OK(hipMemcpyAsync(sphi, phi, n * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
  HIP_OK(hipStreamSynchronize(ctx->stream));
  ctx->soft_B = B;
  ctx->soft_N = N;
  ctx->mpc_last.B = 0;
  return 0;
}

int tmpc_get_soft_state(tmpc_ctx* ctx, int B, int N, double* mu, double* lam, double* phi) {
  if (!ctx) return -1;
  if (ctx->soft_B != B || ctx->soft_N != N)
    return fail(ctx, "no soft-constraint state for B=%d N=%d (solve or tmpc_set_soft_state first)", B, N);
  hipSetDevice(ctx->device);
  const size_t n = (size_t)B * N * 6 * ctx->hmodel.n;
  if (mu) HIP_OK(hipMemcpy(mu, ctx->soft_mu, n * sizeof(double), hipMemcpyDeviceToHost));
  if (lam) HIP_OK(hipMemcpy(lam, ctx->soft_lam, n * sizeof(double), hipMemcpyDeviceToHost));
  if (phi) HIP_OK(hipMemcpy(phi, ctx->soft_phi, n * sizeof(double), hipMemcpyDeviceToHost));
  return 0;
}

int tmpc_set_options(tmpc_ctx* ctx, const tmpc_options* o) {
  if (!ctx || !o) return -1;
  if (o->max_iter_linSys < 1 || o->max_iter_SQP_DDP < 1 || o->max_iter_softConstraints < 1)
    return fail(ctx, "max_iter options must be >= 1");
  if (!(o->alpha_factor_SQP_DDP > 0.0 && o->alpha_factor_SQP_DDP < 1.0))
    return fail(ctx, "alpha_factor_SQP_DDP must be in (0, 1)");
  if (o->precision < TMPC_PRECISION_F64 || o->precision > TMPC_PRECISION_MIXED)
    return fail(ctx, "precision %d (valid: 0 F64, 1 F32, 2 MIXED)", o->precision);
  ctx->opts = *o;
  ctx->mpc_last.B = 0;   // (pcg_warm_start, the precision: an MPC step loop keeps its options)
  return 0;
}

int tmpc_sqp_solve_batch_device(tmpc_ctx* ctx, int B, int N, double dt, int linsys, double* d_x, double* d_u,
                                int32_t* exit_sqp, int32_t* sqp_iter) {
  if (!ctx) return -1;
  hipSetDevice(ctx->device);
  int rc = sqp_device(ctx, B, N, dt, linsys, d_x, d_u, nullptr);
  if (rc) return rc;
  return read_status(ctx, B, exit_sqp, sqp_iter);
}

int tmpc_sqp_solve_batch(tmpc_ctx* ctx, int B, int N, double dt, int linsys, double* x, double* u,
                         int32_t* exit_sqp, int32_t* exit_soft, int32_t* outer_iter, int32_t* sqp_iter,
                         tmpc_trace* trace) {
  if (!ctx) return -1;
  const bool hard_trace = trace && trace->hard_active && ctx->hlim.any_hard;
  return solve_host(ctx, B, N, true, x, u, exit_sqp, exit_soft, outer_iter, sqp_iter, trace, hard_trace,
                    [&](double* d_x, double* d_u, TraceDev* tr) {
                      return sqp_device(ctx, B, N, dt, linsys, d_x, d_u, tr, false, hard_trace);
                    });
}

int tmpc_ilqr_solve_batch(tmpc_ctx* ctx, int B, int N, double dt, double* x, double* u, int32_t* exit_code,
                          int32_t* exit_soft, int32_t* outer_iter, int32_t* iters, tmpc_trace* trace) {
  if (!ctx) return -1;
  return solve_host(ctx, B, N, false, x, u, exit_code, exit_soft, outer_iter, iters, trace, false,
                    [&](double* d_x, double* d_u, TraceDev* tr) { return ilqr_device(ctx, B, N, dt, d_x, d_u, tr); });
}

int tmpc_ilqr_solve_batch_device(tmpc_ctx* ctx, int B, int N, double dt, double* d_x, double* d_u,
                                 int32_t* exit_code, int32_t* iters) {
  if (!ctx) return -1;
  hipSetDevice(ctx->device);
  int rc = ilqr_device(ctx, B, N, dt, d_x, d_u, nullptr);
  if (rc) return rc;
  return read_status(ctx, B, exit_code, iters);
}

// ------------------------------------------------------------------ continuous batching (include/tmpc.h, ABI 10)
int tmpc_sqp_solve_stream_device(tmpc_ctx* ctx, int N, double dt, int linsys, const tmpc_stream* stream) {
  if (!ctx) return -1;
  if (precond_of(linsys) < 0)
    return fail(ctx, "linear system method %d is not available on the GPU (use S/PCG-J/BJ/SS = 1/2/3/4)", linsys);
  return stream_solve(ctx, N, dt, linsys, stream);
}

int tmpc_ilqr_solve_stream_device(tmpc_ctx* ctx, int N, double dt, const tmpc_stream* stream) {
  if (!ctx) return -1;
  return stream_solve(ctx, N, dt, -1, stream);
}

int tmpc_mpc_batch_device(tmpc_ctx* ctx, int B, int N, double dt, int solver, int steps, double* d_x, double* d_u,
                          double* d_x_exec, double* d_u_exec, int32_t* d_exit_codes, int32_t* d_iters) {
  if (!ctx) return -1;
  hipSetDevice(ctx->device);
  return mpc_device(ctx, B, N, dt, solver, steps, d_x, d_u, d_x_exec, d_u_exec, d_exit_codes, d_iters);
}

int tmpc_mpc_batch(tmpc_ctx* ctx, int B, int N, double dt, int solver, int steps, double* x, double* u,
                   double* x_exec, double* u_exec, int32_t* exit_codes, int32_t* iters) {
  if (!ctx) return -1;
  int rc = check_ready(ctx, B, N, solver != TMPC_SOLVER_ILQR);
  if (rc) return rc;
  if (!x || !u || steps < 1) return fail(ctx, "null x/u or steps < 1");
  hipSetDevice(ctx->device);
  const int nx = ctx->hcost.nx, nu = ctx->hcost.nu;
  const size_t xn = (size_t)B * nx * N, un = (size_t)B * nu * (N - 1);
  BUF(double, mpc_x, xn);
  BUF(double, mpc_u, un);
  BUF(double, mpc_xe, (size_t)B * nx * (steps + 1));
  BUF(double, mpc_ue, (size_t)B * nu * steps);
  BUF(int, mpc_codes, (size_t)B * steps);
  BUF(int, mpc_iters, (size_t)B * steps);
  HIP_OK(hipMemcpyAsync(mpc_x, x, xn * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
  HIP_OK(hipMemcpyAsync(mpc_u, u, un * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
  if ((rc = mpc_device(ctx, B, N, dt, solver, steps, mpc_x, mpc_u, mpc_xe, mpc_ue, mpc_codes, mpc_iters))) return rc;
  HIP_OK(hipMemcpy(x, mpc_x, xn * sizeof(double), hipMemcpyDeviceToHost));
  HIP_OK(hipMemcpy(u, mpc_u, un * sizeof(double), hipMemcpyDeviceToHost));
  if (x_exec) HIP_OK(hipMemcpy(x_exec, mpc_xe, sizeof(double) * B * nx * (steps + 1), hipMemcpyDeviceToHost));
  if (u_exec) HIP_OK(hipMemcpy(u_exec, mpc_ue, sizeof(double) * B * nu * steps, hipMemcpyDeviceToHost));
  if (exit_codes) HIP_OK(hipMemcpy(exit_codes, mpc_codes, sizeof(int) * B * steps, hipMemcpyDeviceToHost));
  if (iters) HIP_OK(hipMemcpy(iters, mpc_iters, sizeof(int) * B * steps, hipMemcpyDeviceToHost));
  return 0;
}

int tmpc_mpc_step_device(tmpc_ctx* ctx, int B, int N, double dt, int solver, int step, double* d_x, double* d_u,
                         const tmpc_mpc_io* io) {
  if (!ctx) return -1;
  hipSetDevice(ctx->device);
  return mpc_step_device(ctx, B, N, dt, solver, step, d_x, d_u, io ? *io : tmpc_mpc_io{});
}

int tmpc_mpc_step(tmpc_ctx* ctx, int B, int N, double dt, int solver, int step, double* x, double* u,
                  const tmpc_mpc_io* io) {
  if (!ctx) return -1;
  int rc = check_ready(ctx, B, N, solver != TMPC_SOLVER_ILQR);
  if (rc) return rc;
  if (!x || !u) return fail(ctx, "null x/u");
  hipSetDevice(ctx->device);
  const tmpc_mpc_io h = io ? *io : tmpc_mpc_io{};
  const int nx = ctx->hcost.nx, nu = ctx->hcost.nu;
  const size_t xn = (size_t)B * nx * N, un = (size_t)B * nu * (N - 1);
  BUF(double, step_x, xn);
  BUF(double, step_u, un);
  BUF(double, step_xm, (size_t)B * nx);
  BUF(double, step_u0, (size_t)B * nu);
  BUF(double, step_xp, (size_t)B * nx);
  BUF(int, step_status, (size_t)B * 2);
  HIP_OK(hipMemcpyAsync(step_x, x, xn * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
  HIP_OK(hipMemcpyAsync(step_u, u, un * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
  if (h.x_meas)
    HIP_OK(hipMemcpyAsync(step_xm, h.x_meas, sizeof(double) * B * nx, hipMemcpyHostToDevice, ctx->stream));
  tmpc_mpc_io d{};
  d.x_meas = h.x_meas ? step_xm : nullptr;
  d.u0 = step_u0; d.x_pred = step_xp; d.status = step_status;
  if ((rc = mpc_step_device(ctx, B, N, dt, solver, step, step_x, step_u, d))) return rc;
  HIP_OK(hipMemcpy(x, step_x, xn * sizeof(double), hipMemcpyDeviceToHost));
  HIP_OK(hipMemcpy(u, step_u, un * sizeof(double), hipMemcpyDeviceToHost));
  if (h.u0) HIP_OK(hipMemcpy(h.u0, step_u0, sizeof(double) * B * nu, hipMemcpyDeviceToHost));
  if (h.x_pred) HIP_OK(hipMemcpy(h.x_pred, step_xp, sizeof(double) * B * nx, hipMemcpyDeviceToHost));
  if (h.status) HIP_OK(hipMemcpy(h.status, step_status, sizeof(int) * B * 2, hipMemcpyDeviceToHost));
  return 0;
}

int tmpc_device_alloc(tmpc_ctx* ctx, size_t bytes, void** ptr) {
  if (!ctx || !ptr) return -1;
  hipSetDevice(ctx->device);
  HIP_OK(hipMalloc(ptr, bytes));
  return 0;
}

int tmpc_device_free(tmpc_ctx* ctx, void* ptr) {
  if (!ctx) return -1;
  hipSetDevice(ctx->device);
  HIP_OK(hipFree(ptr));
  return 0;
}

int tmpc_memcpy_h2d(tmpc_ctx* ctx, void* dst, const void* src, size_t bytes) {
  return copy_sync(ctx, dst, src, bytes, hipMemcpyHostToDevice);
}

int tmpc_memcpy_d2h(tmpc_ctx* ctx, void* dst, const void* src, size_t bytes) {
  return copy_sync(ctx, dst, src, bytes, hipMemcpyDeviceToHost);
}

int tmpc_memcpy_d2d(tmpc_ctx* ctx, void* dst, const void* src, size_t bytes) {
  return copy_sync(ctx, dst, src, bytes, hipMemcpyDeviceToDevice);
}

int tmpc_synchronize(tmpc_ctx* ctx) {
  if (!ctx) return -1;
  hipSetDevice(ctx->device);
  HIP_OK(hipStreamSynchronize(ctx->stream));
  resolve_timings(ctx);
  return 0;
}

int tmpc_kernel_stats(tmpc_ctx* ctx, const char* name, int64_t* launches, double* total_ms) {
  if (!ctx || !name) return -1;
  resolve_timings(ctx);
  auto it = ctx->stats.find(name);
  if (launches) *launches = it == ctx->stats.end() ? 0 : it->second.launches;
  if (total_ms) *total_ms = it == ctx->stats.end() ? 0.0 : it->second.total_ms;
  return 0;
}

int tmpc_kernel_bytes(tmpc_ctx* ctx, const char* name, double* bytes) {
  if (!ctx || !name || !bytes) return -1;
  if (std::string(name) != "hard_pcg") return fail(ctx, "kernel '%s' does not count its bytes (counting: hard_pcg)", name);
  auto it = ctx->kbytes.find(name);
  *bytes = it == ctx->kbytes.end() ? 0.0 : it->second;
  return 0;
}

int tmpc_solve_counters(tmpc_ctx* ctx, int64_t* counters) {
  if (!ctx || !counters) return -1;
  for (int i = 0; i < 4; ++i) counters[i] = ctx->last_counters[i];
  return 0;
}

int tmpc_reset_stats(tmpc_ctx* ctx) {
  if (!ctx) return -1;
  resolve_timings(ctx);
  ctx->stats.clear();
  ctx->kbytes.clear();
  return 0;
}

}  // extern "C"
