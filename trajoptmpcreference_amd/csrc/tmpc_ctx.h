// The context behind the C ABI (include/tmpc.h): configuration, the named device-buffer cache, launch timing,
// and what one call leaves for a later one.  Host-only; shared by the solver drivers (tmpc_solve.cpp) and the
// entry points (tmpc_api.cpp, tmpc_api_qp.cpp).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdio>
#include <map>
#include <string>
#include <vector>

#include "../../include/tmpc.h"
#include "tmpc_internal.h"

namespace tmpc {

struct DevBuf {
  void* ptr = nullptr;
  size_t bytes = 0;
};

struct Stat {
  int64_t launches = 0;
  double total_ms = 0.0;
};

struct PendingTiming {
  std::string name;
  hipEvent_t start, stop;
};

}  // namespace tmpc

struct tmpc_ctx {
  int device = 0;
  hipStream_t stream = nullptr;
  std::string err;
  bool has_model = false, has_cost = false;
  tmpc::ModelDev hmodel{};
  tmpc::CostDev hcost{};
  tmpc::ConstrDev hlim{};
  tmpc::ModelDev* dmodel = nullptr;
  tmpc::CostDev* dcost = nullptr;
  tmpc::ConstrDev* dlim = nullptr;
  int soft_B = -1, soft_N = -1;   // shape of the valid soft-constraint state (-1: none)
  int model_id = 0;               // compiled model (tmpc_models.h) equal to the set model; 0 = runtime model
  tmpc_options opts{};
  std::map<std::string, tmpc::DevBuf> bufs;   // by name: only buf() looks a buffer up
  std::map<std::string, tmpc::Stat> stats;
  std::vector<tmpc::PendingTiming> pending;
  std::vector<hipEvent_t> event_pool;
  int* h_count = nullptr;  // pinned
  int64_t last_counters[4] = {0, 0, 0, 0};
  // What the last solve left on the device for the calls that follow it, set where the buffers are allocated
  // (null until then): its per-problem state (alloc_state), its outer-loop results (outer_alloc), the
  // soft-constraint state (alloc_soft; valid for the shape soft_B, soft_N) and the PCG warm start (sqp_device)
  tmpc::ProbState last_st{};
  int* exit_soft = nullptr;
  int* outer_iter = nullptr;
  double *soft_mu = nullptr, *soft_lam = nullptr, *soft_phi = nullptr;
  double* lam_warm = nullptr;
  // the last tmpc_qp_batch with hard limits (tmpc_qp_hard_info reads its hd_* buffers, hard_dev); cleared by every
  // other user of those buffers (setup_hard) and by a change of the limits, so stale data is refused
  struct { int B, N, dmax, W, rmax; } hard_last{0, 0, 0, 0, 0};   // B = 0: none
  tmpc::HardArgs hard_dev{};              // the hd_* buffers as setup_hard last laid them out
  // the last tmpc_qp_batch (tmpc_qp_last_inputs reads the buffers its QP consumed: Amat, Bmat, cvec and Ginv or
  // soft_Gk); cleared by every other user of those buffers (alloc_work), so stale data is refused.  nj, QF_start:
  // the model and cost of that call, which lay the Ghat blocks out
  struct { int B, N, nj, QF_start; bool soft, banded; } qp_last{0, 0, 0, -1, false, false};   // B = 0: none
  // the last tmpc_mpc_step[_device]: what the warm lambda, the soft constants and QF_start on the device continue
  // (step + 1 of the same loop is the only step accepted next); cleared by every other solve (alloc_state) and
  // by every change of the configuration, so another solve's state is refused
  struct { int B, N, solver, step; double dt; } mpc_last{0, 0, 0, 0, 0.0};   // B = 0: none
  std::map<std::string, double> kbytes;   // bytes beyond registers / LDS of counting kernels since tmpc_reset_stats
  std::vector<tmpc_ctx*> subs;            // a stream's concurrent sub-streams (tmpc_stream.substreams): own HIP
                                          // stream and buffers each, the configuration copied from this context
  // The state reference (tmpc_set_reference): xref [ref_R][nx][ref_M] on the device, ref_R = 0: none (every kernel
  // reads CostDev::xg).  A sub-stream's context borrows its parent's array.  ref_step: the MPC step whose horizon
  // solve runs (the window's first column; 0 outside mpc_device).
  const double* ref_dev = nullptr;
  int ref_R = 0, ref_M = 0, ref_step = 0;
};

namespace tmpc {

inline int vfail(tmpc_ctx* c, const char* fmt, va_list ap) {
  char buf[1024];
  vsnprintf(buf, sizeof(buf), fmt, ap);
  if (c) c->err = buf;
  return -1;
}

inline int fail(tmpc_ctx* c, const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  const int rc = vfail(c, fmt, ap);
  va_end(ap);
  return rc;
}

#define HIP_OK(call)                                                                        \
  do {                                                                                      \
    hipError_t e_ = (call);                                                                 \
    if (e_ != hipSuccess) return fail(ctx, "%s failed: %s", #call, hipGetErrorString(e_)); \
  } while (0)

#define LAUNCH_OK(call)                                                                       \
  do {                                                                                        \
    int r_ = (call);                                                                          \
    if (r_ != 0) return fail(ctx, "unsupported size for %s (code %d)", #call, r_);           \
    hipError_t e_ = hipGetLastError();                                                        \
    if (e_ != hipSuccess) return fail(ctx, "launch %s failed: %s", #call, hipGetErrorString(e_)); \
  } while (0)

inline hipEvent_t get_event(tmpc_ctx* ctx) {
  if (!ctx->event_pool.empty()) {
    hipEvent_t e = ctx->event_pool.back();
    ctx->event_pool.pop_back();
    return e;
  }
  hipEvent_t e;
  if (hipEventCreate(&e) != hipSuccess) return nullptr;
  return e;
}

// RAII timing of one launch on the context stream (options.profile)
struct Timed {
  tmpc_ctx* ctx;
  PendingTiming pt;
  bool on;
  Timed(tmpc_ctx* c, const char* name) : ctx(c), on(c->opts.profile != 0) {
    if (!on) return;
    pt.name = name;
    pt.start = get_event(ctx);
    pt.stop = get_event(ctx);
    hipEventRecord(pt.start, ctx->stream);
  }
  ~Timed() {
    if (!on) return;
    hipEventRecord(pt.stop, ctx->stream);
    ctx->pending.push_back(pt);
  }
};

inline void resolve_timings(tmpc_ctx* ctx) {
  for (auto& p : ctx->pending) {
    float ms = 0.f;
    if (hipEventSynchronize(p.stop) == hipSuccess && hipEventElapsedTime(&ms, p.start, p.stop) == hipSuccess) {
      Stat& s = ctx->stats[p.name];
      s.launches += 1;
      s.total_ms += ms;
    }
    ctx->event_pool.push_back(p.start);
    ctx->event_pool.push_back(p.stop);
  }
  ctx->pending.clear();
}

// The context's device buffer `name`, grown to `count` elements.  The name selects the allocation: two call
// sites that pass the same name share memory.
template <typename T>
T* buf(tmpc_ctx* ctx, const char* name, size_t count) {
  DevBuf& b = ctx->bufs[name];
  const size_t bytes = count * sizeof(T);
  if (b.bytes < bytes) {
    if (b.ptr) hipFree(b.ptr);
    b.ptr = nullptr;
    b.bytes = 0;
    if (hipMalloc(&b.ptr, bytes) != hipSuccess) {
      b.ptr = nullptr;
      return nullptr;
    }
    b.bytes = bytes;
  }
  return static_cast<T*>(b.ptr);
}

#define BUF(T, name, count)                                                            \
  T* name = buf<T>(ctx, #name, (size_t)(count));                                       \
  if (!name) return fail(ctx, "device allocation of %s (%zu elements) failed", #name, \
                         (size_t)(count));

// precision modes (tmpc_options.precision): the dynamics' derivatives (M^-1, RNEA gradient: A_k, B_k) in
// fp32 for F32 and MIXED; the trajectory values (the QP's defects, line-search trials, iLQR rollouts) in
// fp32 for MIXED only -- F32 evaluates every trajectory, cost and merit in fp64, so its exit tests see the
// fp64 objective; the Riccati sweep in fp32 for F32 only; Schur / PCG, merit sums and decisions stay fp64
inline bool dyn32(const tmpc_ctx* ctx) { return ctx->opts.precision != TMPC_PRECISION_F64; }
inline bool val32(const tmpc_ctx* ctx) { return ctx->opts.precision == TMPC_PRECISION_MIXED; }
inline bool ric32(const tmpc_ctx* ctx) { return ctx->opts.precision == TMPC_PRECISION_F32; }

// the model the context's launches run on
inline ModelSel model_sel(const tmpc_ctx* ctx) {
  return ModelSel{ctx->hmodel.n, ctx->hmodel.chain != 0, ctx->model_id, ctx->dmodel};
}

inline SolverOpts solver_opts(const tmpc_options& o) {
  SolverOpts s{};
  s.exit_tol_sqp = o.exit_tolerance_SQP_DDP; s.alpha_factor = o.alpha_factor_SQP_DDP;
  s.alpha_min = o.alpha_min_SQP_DDP; s.rho_factor = o.rho_factor_SQP_DDP; s.rho_min = o.rho_min_SQP_DDP;
  s.rho_max = o.rho_max_SQP_DDP; s.rho_init = o.rho_init_SQP_DDP;
  s.exp_red_min = o.expected_reduction_min_SQP_DDP; s.exp_red_max = o.expected_reduction_max_SQP_DDP;
  s.mu = o.merit_mu; s.max_iter_sqp = o.max_iter_SQP_DDP;
  return s;
}

// alpha schedule of the line search (:606, :712-718): 1, f, f^2, ... while alpha > alpha_min
inline std::vector<double> alpha_list(const tmpc_options& o) {
  std::vector<double> a;
  double al = 1.0;
  a.push_back(al);
  while (al > o.alpha_min_SQP_DDP && a.size() < 64) {
    al *= o.alpha_factor_SQP_DDP;
    a.push_back(al);
  }
  return a;
}

// 0 = method S (direct block-tridiagonal solve, k_btsolve); method N (the dense KKT solve) has the
// same solution and takes the same direct path (include/tmpc.h)
inline int precond_of(int linsys) {
  switch (linsys) {
    case TMPC_LINSYS_S: return 0;
    case TMPC_LINSYS_N: return 0;
    case TMPC_LINSYS_PCG_J: return PRECOND_J;
    case TMPC_LINSYS_PCG_BJ: return PRECOND_BJ;
    case TMPC_LINSYS_PCG_SS: return PRECOND_SS;
    case TMPC_LINSYS_PCG_0: return PRECOND_NONE;
    default: return -1;
  }
}

// A wide model (NJ_FULL < n <= NJMAX joints) runs the dynamics on the runtime model, the SQP with the fused
// register / two-rows-per-lane QP (N * nx <= 1024 rows) and iLQR with the VALU Riccati sweep and the plain
// rollout: fp64, QuadraticCost, no box limits (the MFMA sweep's tiles and the fp32 / soft / hard / HBM-row
// instances exist for up to NJ_FULL joints)
inline int wide_ok(tmpc_ctx* ctx, const char* what) {
  const int n = ctx->hmodel.n;
  if (n <= NJ_FULL) return 0;
  if (ctx->opts.precision != TMPC_PRECISION_F64)
    return fail(ctx, "%s: %d joints run in fp64 only (precision modes up to %d joints)", what, n, NJ_FULL);
  return 0;
}

inline int check_ready(tmpc_ctx* ctx, int B, int N, bool qp = true) {
  if (!ctx) return -1;
  if (!ctx->has_model) return fail(ctx, "no model: call tmpc_set_model first");
  if (ctx->hmodel.n > NJ_FULL) {
    const int n = ctx->hmodel.n;
    if (int rc = wide_ok(ctx, qp ? "SQP" : "iLQR")) return rc;
    if (ctx->hlim.any)
      return fail(ctx, "box constraints with %d joints: supported up to %d joints (the soft / hard limit kernels)", n,
                  NJ_FULL);
    if (ctx->has_cost && ctx->hcost.kind != COST_QUADRATIC) return fail(ctx, "%d joints: QuadraticCost only", n);
    if (qp && N * 2 * n > 1024)
      return fail(ctx, "%d joints: the QP takes N * nx <= 1024 rows (N <= %d; got N = %d)", n, 1024 / (2 * n), N);
  }
  if (!ctx->has_cost) return fail(ctx, "no cost: call tmpc_set_cost_quadratic first");
  if (ctx->hcost.nx != 2 * ctx->hmodel.n || ctx->hcost.nu != ctx->hmodel.n)
    return fail(ctx, "cost sizes (nx=%d, nu=%d) do not match the model (n=%d)", ctx->hcost.nx, ctx->hcost.nu,
                ctx->hmodel.n);
  if (B < 1) return fail(ctx, "batch size must be >= 1 (got %d)", B);
  if (N < 2) return fail(ctx, "N must be >= 2 (got %d)", N);
  return 0;   // QPs past the fused kernel's QP_MAX_ROWS take the banded path (qp_banded)
}

// The QP takes the banded variable-block path of tmpc_hard.hip -- built for hard box constraints --
// with hard limits, and also without them past the fused k_qp's QP_MAX_ROWS (1536) rows: there the
// Schur complement is the same block-tridiagonal S with no constraint rows (every knot's row count 0),
// which the banded kernels solve up to HARD_PCG_MAX_ROWS rows by PCG (and by the direct banded
// elimination up to k_hard_schur's LDS bound, checked in setup_hard), in their own canonical order
// (oracle/hard.py pcg_canonical).
inline bool qp_banded(const tmpc_ctx* ctx, int N) {
  return ctx->hlim.any_hard || N * 2 * ctx->hmodel.n > QP_MAX_ROWS;
}

// ------------------------------------------------------------------ the solver drivers (tmpc_solve.cpp)
// One QP phase (shared by SQP, iLQR and tmpc_qp_batch): the launchers' blocks with what a solve keeps fixed --
// their buffers (alloc_work; gs and qp.jsoft: init_soft, else null; qp.gw: goal_window), the horizon, trajectory
// and per-problem masks (bind_work) -- to which run_dynamics / run_qp add the problem list and, per phase, the
// mode and the outputs it writes from the buffers below
struct Work {
  DynArgs dyn;
  QpArgs qp;
  GinvSoftArgs gs;
  double* xs;      // the start states [B][nx] (dyn.xs), which the drivers write
  double *G, *Sd, *Sl, *gam, *lam, *Pd;
  double *U, *Y;   // method S scratch (k_btsolve)
  const double* guess;               // PCG initial iterate [B][N nx] (nullable)
  double* lam_keep;                  // where the PCG path stores lambda (nullable; warm start)
  HardArgs* hard;                    // hard box constraints: the variable-row QP (tmpc_hard.hip)
  double* Sg;                        // S / P^-1 rows in HBM past 1024 rows (k_qp<..., GM>), else null
  unsigned long long* tr_active;     // hard limits: per-QP active-set bitmasks into the trace (nullable)
  int Wtr;                           // trace row stride
};

int alloc_work(tmpc_ctx* ctx, int B, int N, Work& w, bool with_blocks);
int alloc_state(tmpc_ctx* ctx, int B, ProbState& st);
// the soft-constraint state [B][N][6n] (ctx->soft_mu / soft_lam / soft_phi), at its initial constants unless
// it is the valid state of this shape (fresh: start from the constants regardless); w: the QP's per-knot terms
int alloc_soft(tmpc_ctx* ctx, int B, int N);
int init_soft(tmpc_ctx* ctx, int B, int N, bool fresh, Work* w);
int setup_hard(tmpc_ctx* ctx, int B, int N, int T, int precond, HardArgs& hard, int nj_given = -1,
               int rmax_given = -1);
int collect_hard_work(tmpc_ctx* ctx, const HardArgs& hard);
int run_hard_qp(tmpc_ctx* ctx, int nj, const HardArgs& h);
// the horizon, step, trajectory and st's masks into w's blocks: once per solve, before run_qp / ilqr_sweeps
void bind_work(const tmpc_ctx* ctx, int N, double dt, const double* d_x, const double* d_u, const ProbState& st,
               Work& w);
int run_qp(tmpc_ctx* ctx, int B, int precond, const ProbState& st, Work& w, bool keep_blocks, PList P, int nb);
int sqp_device(tmpc_ctx* ctx, int B, int N, double dt, int linsys, double* d_x, double* d_u, TraceDev* tr_out,
               bool keep_warm = false, bool hard_trace = false, const StreamDev* sd = nullptr);
// One iLQR iteration's sweeps (shared by the iLQR driver and tmpc_ilqr_step_batch): the launchers' block with the
// context's cost, limits and soft state (mu, lam), the alphas and the sweeps' buffers set (ilqr_sweep_setup);
// ilqr_sweeps adds the problems, the trajectory and the dynamics' blocks.
using IlqrSweep = IlqrArgs;
// What iLQR refuses (UrdfCost, hard limits, check_ready's wide-model restrictions), then the sweeps' buffers, the
// soft state (init_soft; fresh: from the limits' initial constants regardless) and the alphas on the stream.
int ilqr_sweep_setup(tmpc_ctx* ctx, int B, int N, bool fresh_soft, IlqrSweep& q);
// run_dynamics, the backward sweep, the T rollouts with their costs (soft values included): the problems of
// P / nb that are st.active, at st.rho
int ilqr_sweeps(tmpc_ctx* ctx, const ProbState& st, const Work& w, PList P, int nb, const IlqrSweep& q);
int ilqr_device(tmpc_ctx* ctx, int B, int N, double dt, double* d_x, double* d_u, TraceDev* tr_out,
                const StreamDev* sd = nullptr);
int stream_solve(tmpc_ctx* ctx, int N, double dt, int linsys, const tmpc_stream* s);
int mpc_device(tmpc_ctx* ctx, int B, int N, double dt, int solver, int steps, double* d_x, double* d_u,
               double* d_xe, double* d_ue, int* d_codes, int* d_iters);
// one step of that loop from a measured state (include/tmpc.h tmpc_mpc_io: device pointers)
int mpc_step_device(tmpc_ctx* ctx, int B, int N, double dt, int solver, int step, double* d_x, double* d_u,
                    const tmpc_mpc_io& io);
// The goal window of a horizon solve (tmpc_internal.h launch_goal_window): null without a reference.  What a
// reference cannot be combined with (UrdfCost; R not 1 or `rows`, the batch size or the stream's period) is
// refused here.  pid / pbase / mask: a stream's slots (null / 0 / null: problem b, every problem).
int goal_window(tmpc_ctx* ctx, int B, int N, int rows, const char* rows_name, const int* pid, int pbase,
                const int* mask, const double** gw);

}  // namespace tmpc
