// The batched solver drivers behind the C ABI (tmpc_api.cpp): SQP, iLQR, their continuous-batching streams
// and the receding-horizon MPC loop.
//
// The SQP driver is the host half of TrajoptMPCReference.SQP
// (TrajoptMPCReference.py:510-760): it launches, per SQP iteration, the
// masked device phases QP-build (dynamics + gradients) -> Schur -> PCG ->
// dxu -> line-search terms -> decision, and stops when no problem of the
// batch is active.  All per-problem branching lives on the device
// (k_ls_decide); the host reads back one integer per iteration.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <thread>
#include <vector>

#include "tmpc_ctx.h"

namespace tmpc {

int ctx_fail(tmpc_ctx* ctx, const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  const int rc = vfail(ctx, fmt, ap);
  va_end(ap);
  return rc;
}
int ctx_device(const tmpc_ctx* ctx) { return ctx->device; }
hipStream_t ctx_stream(const tmpc_ctx* ctx) { return ctx->stream; }

// ------------------------------------------------------------------ QP phase (shared by SQP and tmpc_qp_batch)
// P / nb: the problems the batch launches visit (tmpc_internal.h PList; the identity and B outside the
// lock-step loop)

// the dynamics of the problems that need fresh gradients: defects c_k, M^-1, then A_k, B_k (SQP's QP and iLQR)
static int run_dynamics(tmpc_ctx* ctx, const Work& w, PList P, int nb) {
  const ModelSel m = model_sel(ctx);
  DynArgs a = w.dyn;
  a.P = P; a.B = nb;
  { Timed t(ctx, "qp_fd"); LAUNCH_OK(launch_qp_fd(val32(ctx), ctx->stream, m, a)); }
  { Timed t(ctx, "qp_minv"); LAUNCH_OK(launch_qp_minv(dyn32(ctx), ctx->stream, m, a)); }
  { Timed t(ctx, "qp_grad"); LAUNCH_OK(launch_qp_grad(dyn32(ctx), ctx->stream, m, a)); }
  return 0;
}

void bind_work(const tmpc_ctx* ctx, int N, double dt, const double* d_x, const double* d_u, const ProbState& st,
               Work& w) {
  w.dyn.N = w.qp.N = w.gs.N = N; w.dyn.dt = w.qp.dt = dt; w.dyn.x = w.qp.x = w.gs.x = d_x;
  w.dyn.u = w.qp.u = w.gs.u = d_u; w.dyn.need = st.need_grad; w.qp.active = w.gs.active = st.active; w.gs.rho = st.rho;
  w.qp.C = w.gs.C = ctx->dcost; w.gs.Cs = ctx->dlim;
  w.qp.cost_diag = ctx->hcost.kind == COST_QUADRATIC && ctx->hcost.diag != 0;
}

// the banded QP: rows + layout + Schur band, the solve, dxu
int run_hard_qp(tmpc_ctx* ctx, int nj, const HardArgs& h) {
  { Timed t(ctx, "hard_schur"); LAUNCH_OK(launch_hard_schur(ctx->stream, nj, h)); }
  { Timed t(ctx, h.precond == 0 ? "hard_direct" : "hard_pcg"); LAUNCH_OK(launch_hard_solve(ctx->stream, nj, h)); }
  { Timed t(ctx, "dxu"); LAUNCH_OK(launch_hard_dxu(ctx->stream, nj, h)); }
  return 0;
}

int run_qp(tmpc_ctx* ctx, int B, int precond, const ProbState& st, Work& w, bool keep_blocks, PList P, int nb) {
  const int nj = ctx->hmodel.n, N = w.qp.N;
  const bool soft = w.qp.jsoft != nullptr;
  if (int rc = run_dynamics(ctx, w, P, nb)) return rc;
  {
    Timed t(ctx, "ginv");
    GinvSoftArgs g = w.gs;
    g.P = P; g.B = nb;
    if (soft) LAUNCH_OK(launch_ginv_soft(ctx->stream, nj, g));
    else LAUNCH_OK(launch_ginv(ctx->stream, nj, ctx->dcost, P, nb, st.rho, st.active, w.G));
  }
  // what every phase of the fused QP reads; a phase adds its mode, the PCG's bounds and the outputs it writes
  QpArgs q = w.qp;
  q.P = P; q.B = nb; q.precond = PRECOND_SS; q.G = soft ? w.gs.Gk : w.G;
  if (w.hard) {   // hard box constraints: rows of C per knot, banded S (tmpc_hard.hip)
    HardArgs h = *w.hard;
    h.precond = precond; h.Ghat = q.G; h.per_knot = soft || ctx->hcost.kind == COST_EE; h.A = q.A; h.Bm = q.Bm;
    h.cvec = q.cvec; h.jsoft = q.jsoft; h.x = q.x; h.u = q.u; h.active = st.active; h.iters = q.iters;
    h.dx = q.dx; h.du = q.du; h.tol = ctx->opts.exit_tolerance_linSys; h.max_iter = ctx->opts.max_iter_linSys;
    h.iter = st.iter; h.Wtr = w.Wtr; h.tr_active = w.tr_active;
    HIP_OK(hipMemsetAsync(q.iters, 0, sizeof(int) * B, ctx->stream));
    if (q.gw) {   // tracking: the cost gradient against the goal window, as the banded kernels' gvec input
      BUF(double, hd_gvec, (size_t)B * N * 3 * nj);
      Timed t(ctx, "hard_track_grad");
      LAUNCH_OK(launch_hard_track_grad(ctx->stream, nj, h, q.gw, hd_gvec));
      h.gvec = hd_gvec;
    }
    return run_hard_qp(ctx, nj, h);
  }
  if (precond == 0) {   // method S: Schur blocks -> direct solve -> dxu
    QpArgs a = q;
    a.mode = QP_MODE_SCHUR; a.Sd = w.Sd; a.Sl = w.Sl; a.gam = w.gam;
    { Timed t(ctx, "schur"); LAUNCH_OK(launch_qp(ctx->stream, nj, a)); }
    a.P = PList{}; a.B = B; a.U = w.U; a.Y = w.Y; a.lam = w.lam;   // every problem: k_btsolve takes no problem list
    { Timed t(ctx, "btsolve"); LAUNCH_OK(launch_btsolve(ctx->stream, 2 * nj, a)); }
    a = q;
    a.mode = QP_MODE_DXU; a.lam = w.lam;
    { Timed t(ctx, "dxu"); LAUNCH_OK(launch_qp(ctx->stream, nj, a)); }
    return 0;
  }
  {
    QpArgs a = q;
    a.mode = QP_MODE_PCG; a.precond = precond; a.tol = ctx->opts.exit_tolerance_linSys;
    a.max_iter = ctx->opts.max_iter_linSys; a.guess = w.guess; a.Sg = w.Sg; a.lam = keep_blocks ? w.lam : w.lam_keep;
    if (keep_blocks) { a.Sd = w.Sd; a.Sl = w.Sl; a.gam = w.gam; a.Pd = w.Pd; }
    Timed t(ctx, "qp");
    LAUNCH_OK(launch_qp(ctx->stream, nj, a));
  }
  return 0;
}

int alloc_work(tmpc_ctx* ctx, int B, int N, Work& w, bool with_blocks) {
  const int nj = ctx->hmodel.n, nx = 2 * nj, K = N - 1;
  BUF(double, xs, (size_t)B * nx);
  BUF(double, qdd, (size_t)B * K * nj);
  BUF(double, minv, (size_t)B * K * nj * nj);
  BUF(double, cvec, (size_t)B * N * nx);
  BUF(double, Amat, (size_t)B * K * nx * nx);
  BUF(double, Bmat, (size_t)B * K * nx * nj);
  BUF(double, Ginv, (size_t)B * 3 * nx * nx);
  BUF(double, dx, (size_t)B * N * nx);
  BUF(double, du, (size_t)B * K * nj);
  BUF(int, iters, (size_t)B);
  ctx->qp_last = {0, 0, 0, -1, false, false};   // these buffers are about to be rewritten (tmpc_qp_last_inputs)
  w = Work{};   // everything else null until its user sets it
  w.dyn.xs = w.xs = xs; w.dyn.qdd = qdd; w.dyn.minv = minv; w.qp.cvec = w.dyn.cvec = cvec; w.qp.A = w.dyn.A = Amat;
  w.qp.Bm = w.dyn.Bm = Bmat; w.G = Ginv; w.qp.dx = dx; w.qp.du = du; w.qp.iters = iters;
  if (N * nx >= qp_gm_min_rows() && !qp_banded(ctx, N)) {   // the GM QP kernel's rows of S / P^-1
    BUF(double, qp_gm, qp_gm_doubles(B, N, nx));
    w.Sg = qp_gm;
  }
  if (with_blocks) {
    BUF(double, Sdiag, (size_t)B * N * nx * nx);
    BUF(double, Slo, (size_t)B * (K > 0 ? K : 1) * nx * nx);
    BUF(double, gam, (size_t)B * N * nx);
    BUF(double, lam, (size_t)B * N * nx);
    BUF(double, Pdiag, (size_t)B * N * nx * nx);
    w.Sd = Sdiag;
    w.Sl = Slo;
    w.gam = gam;
    w.lam = lam;
    w.Pd = Pdiag;
    BUF(double, btU, (size_t)B * (K > 0 ? K : 1) * nx * nx);
    BUF(double, btY, (size_t)B * N * nx);
    w.U = btU;
    w.Y = btY;
  }
  return 0;
}

int goal_window(tmpc_ctx* ctx, int B, int N, int rows, const char* rows_name, const int* pid, int pbase,
                const int* mask, const double** gw) {
  *gw = nullptr;
  if (!ctx->ref_R) return 0;
  if (ctx->hcost.kind == COST_EE)
    return fail(ctx, "a state reference (tmpc_set_reference) with UrdfCost: the task-space goal stays constant; "
                "clear the reference (tmpc_set_reference with R = 0)");
  if (ctx->ref_R != 1 && ctx->ref_R != rows)
    return fail(ctx, "reference rows R = %d: must be 1 or the %s (%d)", ctx->ref_R, rows_name, rows);
  const int nx = 2 * ctx->hmodel.n;
  BUF(double, goal_win, (size_t)B * N * nx);
  GoalWindowArgs a{};
  a.B = B; a.N = N; a.nx = nx; a.R = ctx->ref_R; a.M = ctx->ref_M; a.step = ctx->ref_step; a.xref = ctx->ref_dev;
  a.pid = pid; a.pbase = pbase; a.mask = mask; a.gw = goal_win;
  launch_goal_window(ctx->stream, a);
  HIP_OK(hipGetLastError());
  *gw = goal_win;
  return 0;
}

int alloc_state(tmpc_ctx* ctx, int B, ProbState& st) {
  BUF(double, st_rho, B);
  BUF(double, st_drho, B);
  BUF(double, st_J, B);
  BUF(double, st_c, B);
  BUF(double, st_merit, B);
  BUF(int, st_iter, B);
  BUF(int, st_active, B);
  BUF(int, st_need, B);
  BUF(int, st_exit, B);
  st = ProbState{};
  st.rho = st_rho; st.drho = st_drho; st.J = st_J; st.c = st_c; st.merit = st_merit;
  st.iter = st_iter; st.active = st_active; st.need_grad = st_need; st.exit_sqp = st_exit;
  ctx->last_st = st;
  ctx->mpc_last.B = 0;   // a solve begins: an MPC step loop continues only where mpc_step_device records it again
  return 0;
}

static int alloc_trace(tmpc_ctx* ctx, int B, int W, TraceDev& tr) {
  BUF(int, tr_iteration, (size_t)B * W);
  BUF(int, tr_ls, (size_t)B * W);
  BUF(double, tr_alpha, (size_t)B * W);
  BUF(double, tr_rho, (size_t)B * W);
  BUF(double, tr_J, (size_t)B * W);
  BUF(double, tr_c, (size_t)B * W);
  BUF(double, tr_merit, (size_t)B * W);
  BUF(double, tr_D, (size_t)B * W);
  BUF(double, tr_ratio, (size_t)B * W);
  BUF(int, tr_acc, (size_t)B * W);
  BUF(int, tr_pcg, (size_t)B * W);
  BUF(int, tr_sing, (size_t)B * W);
  HIP_OK(hipMemsetAsync(tr_sing, 0, (size_t)B * W * sizeof(int), ctx->stream));   // iLQR never sets it
  tr = TraceDev{};   // hard_active: null unless the solve records it
  tr.iteration = tr_iteration; tr.ls_iter = tr_ls; tr.alpha = tr_alpha; tr.rho = tr_rho; tr.J = tr_J; tr.c = tr_c;
  tr.merit = tr_merit; tr.D = tr_D; tr.ratio = tr_ratio; tr.accepted = tr_acc; tr.pcg_iters = tr_pcg;
  tr.singular = tr_sing;
  return 0;
}

// soft-constraint state [B][N][6n] (mu, lambda, phi)
int alloc_soft(tmpc_ctx* ctx, int B, int N) {
  const size_t n = (size_t)B * N * 6 * ctx->hmodel.n;
  BUF(double, soft_mu, n);
  BUF(double, soft_lam, n);
  BUF(double, soft_phi, n);
  ctx->soft_mu = soft_mu;
  ctx->soft_lam = soft_lam;
  ctx->soft_phi = soft_phi;
  return 0;
}

int init_soft(tmpc_ctx* ctx, int B, int N, bool fresh, Work* w) {
  const int nj = ctx->hmodel.n, nx = 2 * nj;
  if (int rc = alloc_soft(ctx, B, N)) return rc;
  if (fresh || ctx->soft_B != B || ctx->soft_N != N) {
    launch_soft_init(ctx->stream, ctx->dlim, (size_t)B * N * 6 * nj, 6 * nj, ctx->soft_mu, ctx->soft_lam,
                     ctx->soft_phi);
    HIP_OK(hipGetLastError());
    ctx->soft_B = B;
    ctx->soft_N = N;
  }
  if (w) {
    BUF(double, soft_Gk, (size_t)B * N * (nx * nx + nj * nj));
    BUF(double, soft_j, (size_t)B * N * (nx + nj));
    w->gs.Gk = soft_Gk;
    w->gs.jsoft = soft_j;
    w->qp.jsoft = soft_j;
    w->gs.mu = ctx->soft_mu;
    w->gs.lam = ctx->soft_lam;
  }
  return 0;
}

// Buffers of the hard-constraint QP (tmpc_hard.hip) for B problems of N knots; T line-search trials.
// nj_given / rmax_given >= 0: the plugin-hook QP's joint count and rows per knot (its rows come from the
// caller's constraint hooks, not from the context's limits)
int setup_hard(tmpc_ctx* ctx, int B, int N, int T, int precond, HardArgs& hard, int nj_given, int rmax_given) {
  const int nj = nj_given >= 0 ? nj_given : ctx->hmodel.n, nx = 2 * nj;
  // rows per knot, at most: FULL_SET both bounds of every entry; ACTIVE_SET one per entry when lb < ub
  // (z - lb < 0 and ub - z < 0 cannot hold together), else both
  int rmax = 0;
  bool full = false;
  for (int t = 0; t < 3 && rmax_given < 0; ++t) {
    if (ctx->hlim.hard[t] == HARD_NONE) continue;
    bool ordered = ctx->hlim.hard[t] == HARD_ACTIVE;
    for (int i = 0; i < nj; ++i) ordered = ordered && ctx->hlim.lb[t][i] < ctx->hlim.ub[t][i];
    rmax += ordered ? nj : 2 * nj;
    if (ctx->hlim.hard[t] == HARD_FULL) full = true;
  }
  if (rmax_given >= 0) rmax = rmax_given;
  if (full && precond != 0)
    return fail(ctx, "FULL_SET box constraints with a PCG method: the inactive rows of C are zero, so S is "
                "singular and the reference's preconditioner raises LinAlgError (PCG.py:168-188); use method S");
  ctx->hard_last = {0, 0, 0, 0, 0};           // the hd_* buffers are about to be reused: no stale QP info
  hard = HardArgs{};
  hard.B = B;
  hard.N = N;
  hard.rmax = rmax;
  hard.dmax = nx * N + N * hard.rmax;
  const int gmax = nx + 2 * hard.rmax;         // the last group holds two knots' hard rows
  hard.W = 2 * gmax - 1;
  if (precond != 0 && hard.dmax > HARD_PCG_MAX_ROWS)
    return fail(ctx, "%s: Schur dimension up to %d exceeds the banded PCG's %d rows (methods S / N go further)",
                ctx->hlim.any_hard || rmax_given > 0 ? "hard constraints" : "N * nx past the fused QP's rows",
                hard.dmax, HARD_PCG_MAX_ROWS);
  if (hard.W > 1024) return fail(ctx, "hard constraints: band half-width %d > 1024", hard.W);
  if (hard_schur_lds_bytes(N, nj, hard.dmax) > CU_LDS_BYTES) {
    // the largest N whose k_hard_schur LDS fits: N (24 nj + 8) + 8 (nx + rmax) N + 72 nj^2 (+ 12 of rounding)
    int nmax = N;
    while (nmax > 2 && hard_schur_lds_bytes(nmax, nj, nx * nmax + nmax * hard.rmax) > CU_LDS_BYTES) --nmax;
    return fail(ctx, "%s: N = %d needs %zu bytes of LDS in the banded Schur kernel (k_hard_schur), more than a "
                "CU's %zu; the largest supported horizon for this robot%s is N = %d",
                ctx->hlim.any_hard ? "hard constraints" : "N * nx past the fused QP's rows", N,
                hard_schur_lds_bytes(N, nj, hard.dmax), CU_LDS_BYTES,
                ctx->hlim.any_hard ? " and these limits" : "", nmax);
  }
  const size_t BW = 2 * (size_t)hard.W + 1, nbmax = hard.dmax / nx + 1;
  hard.Cs = ctx->dlim;
  hard.C = ctx->dcost;
  const int rbuf = hard.rmax > 0 ? hard.rmax : 1;   // no hard limits (the banded path past QP_MAX_ROWS): rmax = 0
  BUF(int, hd_cnt, (size_t)B * N);
  BUF(int, hd_col, (size_t)B * N * rbuf);
  BUF(double, hd_sgn, (size_t)B * N * rbuf);
  BUF(double, hd_val, (size_t)B * N * rbuf);
  BUF(int, hd_roff, (size_t)B * N);
  BUF(int, hd_hoff, (size_t)B * N);
  BUF(int, hd_dim, (size_t)B);
  BUF(int, hd_rkind, (size_t)B * hard.dmax);
  BUF(int, hd_rknot, (size_t)B * hard.dmax);
  BUF(int, hd_ridx, (size_t)B * hard.dmax);
  BUF(int, hd_slot, (size_t)B * N * rbuf);
  BUF(unsigned long long, hd_amask, (size_t)B * N);
  BUF(int, hd_sing, (size_t)B);
  HIP_OK(hipMemsetAsync(hd_sing, 0, (size_t)B * sizeof(int), ctx->stream));
  hard.hslot = hd_slot; hard.amask = hd_amask; hard.sing = hd_sing;
  BUF(int, hd_rng, (size_t)B * hard.dmax * 2);
  hard.rng = hd_rng;
  BUF(double, hd_Y, (size_t)B * hard.dmax * 2 * (nx + nj));
  BUF(double, hd_Sb, (size_t)B * hard.dmax * BW);
  BUF(double, hd_gam, (size_t)B * hard.dmax);
  BUF(double, hd_lam, (size_t)B * hard.dmax);
  hard.cnt = hd_cnt; hard.hcol = hd_col; hard.hsgn = hd_sgn; hard.hval = hd_val;
  hard.roff = hd_roff; hard.hoff = hd_hoff; hard.dim = hd_dim;
  hard.rkind = hd_rkind; hard.rknot = hd_rknot; hard.ridx = hd_ridx;
  hard.Y = hd_Y; hard.Sb = hd_Sb; hard.gam = hd_gam; hard.lam = hd_lam;
  ctx->hard_dev = hard;   // what tmpc_qp_hard_info reads once a QP has run on them (hard_last)
  if (precond == 0) {
    BUF(double, hd_M, (size_t)B * hard.dmax * BW);
    BUF(double, hd_rhs, (size_t)B * hard.dmax);
    hard.M = hd_M;
    hard.rhs = hd_rhs;
  } else {
    BUF(double, hd_Pd, (size_t)B * nbmax * nx * nx);
    BUF(double, hd_Pl, (size_t)B * nbmax * nx * nx);
    BUF(double, hd_Ptr, (size_t)B * nbmax * nx * nx);
    hard.Pd = hd_Pd; hard.Pl = hd_Pl; hard.Ptr = hd_Ptr;
  }
  BUF(double, hd_terms, (size_t)B * (T > 0 ? T : 1) * N);
  hard.hterms = hd_terms;
  if (precond != 0) {
    BUF(double, hd_work, (size_t)B);
    HIP_OK(hipMemsetAsync(hd_work, 0, (size_t)B * sizeof(double), ctx->stream));
    hard.work = hd_work;
  }
  return 0;
}

// add the per-problem algorithmic bytes k_hard_pcg counted in this solve to ctx->kbytes["hard_pcg"]
int collect_hard_work(tmpc_ctx* ctx, const HardArgs& hard) {
  if (!hard.work) return 0;
  std::vector<double> w(hard.B);
  HIP_OK(hipMemcpyAsync(w.data(), hard.work, sizeof(double) * hard.B, hipMemcpyDeviceToHost, ctx->stream));
  HIP_OK(hipStreamSynchronize(ctx->stream));
  double sum = 0.0;
  for (double v : w) sum += v;
  ctx->kbytes["hard_pcg"] += sum;
  return 0;
}

// the hard box-constraint terms of the merit's violation at the line-search trial points
static int hard_ls(tmpc_ctx* ctx, int nj, const HardArgs& base, int B, int N, int T, const double* alphas, const double* x,
                   const double* u, double* dx, double* du, const int* active) {
  HardArgs h = base;
  h.B = B; h.N = N; h.T = T; h.alphas = alphas; h.x = x; h.u = u; h.dx = dx; h.du = du; h.active = active;
  return launch_hard_ls(ctx->stream, nj, h);
}

// The problem list of the lock-step loop: mask = the per-problem "may still do work" flag (st.active
// without soft limits, outer_active with them: both only ever go 1 -> 0 inside the loop), idx / cnt
// its device list, P / nb what the iteration's launches take (tmpc_internal.h PList).
struct AliveList {
  const int* mask;
  int* idx;
  int* cnt;
  int B;
  PList P;
  int nb;
};

static int alloc_alive(tmpc_ctx* ctx, int B, const int* mask, AliveList& al) {
  BUF(int, alive_idx, B);
  BUF(int, alive_cnt, 1);
  al = AliveList{};   // P: the identity until the loop builds the list
  al.mask = mask; al.idx = alive_idx; al.cnt = alive_cnt; al.B = B; al.nb = B;
  return 0;
}

// Lock-step batch loop with a lag-1 termination test.  Each batch iteration writes its two flags
// (some problem continues its inner loop / some problem restarted an outer pass) and the length of
// the rebuilt problem list into its own slot of active_count[2][4]; the host copies them to pinned
// memory and tests iteration `it` only after iteration `it + 1` has been enqueued, so the GPU never
// idles while the host decides.  Every kernel masks itself with the per-problem state, so the one
// iteration enqueued after the batch finished is a no-op for every problem (need_grad / active /
// outer_active are all 0).  The launches of iteration `it` visit the problem list built at the end
// of `it - 1` (on the stream, so exact), with the grid sized by the list length the host last read,
// the one of iteration `it - 2` (an upper bound because the list only shrinks: the masks go 1 -> 0 inside
// the loop and never back -- k_alive_list flags any growth and the loop then fails instead of silently
// skipping problems); the tail of a batch whose problems converge at different iterations then
// dispatches only its live problems' workgroups.
template <class Body>
static int lockstep_loop(tmpc_ctx* ctx, long cap, int* active_count, AliveList& al, Body body) {
  hipEvent_t ev[2] = {get_event(ctx), get_event(ctx)};
  if (!ev[0] || !ev[1]) return fail(ctx, "hipEventCreate failed");
  int rc = 0;
  launch_alive_list(ctx->stream, al.B, al.mask, al.idx, al.cnt);
  HIP_OK(hipGetLastError());
  al.P = PList{al.idx, al.cnt};
  al.nb = al.B;
  for (long it = 0; it < cap; ++it) {
    const int p = (int)(it & 1);
    int* ac = active_count + 4 * p;
    if (it >= 2) al.nb = std::max(1, std::min(al.nb, ctx->h_count[4 * p + 2]));   // synced at it - 1
    HIP_OK(hipMemsetAsync(ac, 0, 4 * sizeof(int), ctx->stream));
    if ((rc = body(ac))) break;
    launch_alive_list(ctx->stream, al.B, al.mask, al.idx, al.cnt, ac + 2);
    HIP_OK(hipGetLastError());
    HIP_OK(hipMemcpyAsync(ctx->h_count + 4 * p, ac, 4 * sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
    HIP_OK(hipEventRecord(ev[p], ctx->stream));
    if (it > 0) {
      HIP_OK(hipEventSynchronize(ev[p ^ 1]));
      const int* h = ctx->h_count + 4 * (p ^ 1);
      if (h[3] != 0) {   // k_alive_list: the list grew, so a grid sized by an older length skipped problems
        rc = fail(ctx, "internal: the problem list of the lock-step loop grew (a problem re-entered its loop); "
                  "the grid-size bound no longer holds");
        break;
      }
      if (h[0] == 0 && h[1] == 0) break;
    }
  }
  al.P = PList{nullptr, nullptr};
  al.nb = al.B;
  ctx->event_pool.push_back(ev[0]);
  ctx->event_pool.push_back(ev[1]);
  return rc;
}

// ------------------------------------------------------------------ the outer loop SQP and iLQR share
// What both solvers run on: the QP / dynamics buffers, the per-problem state and trace, the outer
// (soft-constraint) loop's state and the lock-step loop's problem list.
struct Outer {
  Work w;
  ProbState st;
  TraceDev tr;
  int* active_count;   // [2][4] (lag-1 double buffer): [0] some problem in its inner loop, [1] some problem restarted a pass, [2] problem-list length
  unsigned long long* counters;
  SoftOuterArgs so;   // the outer loop's block: its state (outer_alloc) and the soft state the solver runs on (mu, lam,
                      // phi: its caller sets them; null: none); outer_run adds the rest
  bool soft;          // soft box limits
  bool per_problem;   // the outer loop per problem (k_soft_outer with act_init): soft limits, and every stream (a slot's
                      // problem is finished when it leaves its outer loop, which without soft limits is
                      // check_and_update's exit 1)
  AliveList alv;
};

// Allocation only, but for alloc_trace's memset: nothing else goes onto the stream here.
static int outer_alloc(tmpc_ctx* ctx, int B, int N, bool with_blocks, bool stream, Outer& o) {
  int rc;
  if ((rc = alloc_work(ctx, B, N, o.w, with_blocks))) return rc;
  if ((rc = alloc_state(ctx, B, o.st))) return rc;
  if ((rc = alloc_trace(ctx, B, ctx->opts.max_iter_SQP_DDP + 1, o.tr))) return rc;
  BUF(int, active_count, 8);
  BUF(unsigned long long, counters, 4);
  BUF(int, outer_active, B);
  BUF(int, outer_iter, B);
  BUF(int, exit_soft, B);
  o.active_count = active_count;
  o.counters = counters;
  o.so.outer_active = outer_active;
  o.so.outer_iter = ctx->outer_iter = outer_iter;
  o.so.exit_soft = ctx->exit_soft = exit_soft;
  o.soft = ctx->hlim.any != 0;
  o.per_problem = o.soft || stream;
  return alloc_alive(ctx, B, o.per_problem ? outer_active : o.st.active, o.alv);
}

// The solve, from the point where the slots hold their starting trajectories.
//   init(mask, ac, activate): initial cost / merit of the problems in `mask` (st.active: all; act_init: restarted
//     passes and a stream's new problems, which the decide kernel then moves into their inner loop: activate =
//     st.active)
//   iteration(ac): one iteration of every problem in its inner loop; ac[0] = some problem continues
//   sd (nullable): the stream whose finished slots k_soft_outer hands on; lam_keep: the stream's PCG warm start
//   prob_counters: the decide kernels' per-problem tallies [B][3]; T: line-search trials (solve counter 3)
// Unconstrained batches run one inner loop in lock-step; with soft limits, and in every stream, the outer loop
// (:531-757) runs per problem: a problem whose inner loop exits runs check_and_update_soft_constraints at once
// (k_soft_outer, per-problem mode) and starts its next pass the following iteration, while the rest of the batch
// carries on.  Launches per solve: the largest per-problem total of iterations, not the sum over passes of each
// pass's slowest problem (BASELINE config 4: 657 -> see DESIGN.md).  Each problem's own sequence of operations is
// the lock-step one, so its results are identical.
template <class Init, class Iteration>
static int outer_run(tmpc_ctx* ctx, int B, int N, Outer& o, double* d_x, double* d_u, const StreamDev* sd,
                     double* lam_keep, unsigned long long* prob_counters, int T, Init init, Iteration iteration) {
  const int nj = ctx->hmodel.n, nx = 2 * nj;
  const tmpc_options& op = ctx->opts;
  int rc;
  // xs = x[:, 0] (:527)
  HIP_OK(hipMemcpy2DAsync(o.w.xs, sizeof(double), d_x, (size_t)N * sizeof(double), sizeof(double), (size_t)B * nx,
                          hipMemcpyDeviceToDevice, ctx->stream));
  launch_outer_init(ctx->stream, B, o.so.outer_active, o.so.outer_iter, o.so.exit_soft);
  launch_init_state(ctx->stream, B, op.rho_init_SQP_DDP, o.st, o.so.outer_active);
  HIP_OK(hipMemsetAsync(o.active_count, 0, 8 * sizeof(int), ctx->stream));
  if ((rc = init(o.st.active, o.active_count, nullptr))) return rc;
  SoftOuterArgs& sa = o.so;   // check_and_update_soft_constraints; a launch adds its problems and its flag slot
  sa.Cs = ctx->dlim; sa.N = N; sa.nj = nj; sa.tol = op.exit_tolerance_softConstraints;
  sa.max_iter = op.max_iter_softConstraints; sa.x = d_x; sa.u = d_u;
  if (!o.per_problem) {
    // one inner loop (at most max_iter iterations, + 1 for the lag of the exit test);
    // check_and_update_soft_constraints then exits 1 (:531-757)
    rc = lockstep_loop(ctx, (long)op.max_iter_SQP_DDP + 1, o.active_count, o.alv, iteration);
    if (rc) return rc;
    sa.B = B; sa.outer_count = o.active_count;
    launch_soft_outer(ctx->stream, sa);
    HIP_OK(hipGetLastError());
  } else {
    BUF(int, act_init, B);
    HIP_OK(hipMemsetAsync(act_init, 0, sizeof(int) * B, ctx->stream));
    const long per = (long)(op.max_iter_softConstraints + 1) * (op.max_iter_SQP_DDP + 1) + 3;
    // a stream: every batch iteration advances some problem by one iteration, so P x per bounds it
    const long cap = sd ? per * sd->P + 3 : per;
    // the outer loop per problem, and a stream's hand-over of finished slots
    sa.st = o.st; sa.act_init = act_init; sa.rho_init = op.rho_init_SQP_DDP; sa.xs = o.w.xs; sa.tr = o.tr;
    sa.lam_warm = lam_keep;
    if (sd) sa.sd = *sd;
    rc = lockstep_loop(ctx, cap, o.active_count, o.alv, [&](int* ac) -> int {
      int r = iteration(ac);
      if (r) return r;
      {   // a stream: k_soft_outer also hands finished slots on (finished problems out, pending ones in)
        Timed t(ctx, "soft_outer");
        sa.P = o.alv.P; sa.B = o.alv.nb; sa.outer_count = ac + 1;
        launch_soft_outer(ctx->stream, sa);
        HIP_OK(hipGetLastError());
        // tracking: the goals of the problems that just entered a slot (act_init), into the solve's window (a
        // stream runs outside the MPC loop, so ctx->ref_step is 0: the reference's first column)
        if (sd && o.w.qp.gw && (r = goal_window(ctx, B, N, sd->period, "stream's period", sd->slot_pid, sd->pbase,
                                                act_init, &o.w.qp.gw)))
          return r;
      }
      // restarted passes (act_init, set by k_soft_outer) and a stream's new problems: initial cost / merit, then
      // into the inner loop; masked by act_init, so a no-op when no pass restarted
      Timed t(ctx, "init_merit");
      return init(act_init, ac, o.st.active);
    });
    if (rc) return rc;
  }
  launch_sum_counters(ctx->stream, B, prob_counters, o.counters);
  unsigned long long hc[4] = {0, 0, 0, 0};
  HIP_OK(hipMemcpyAsync(hc, o.counters, sizeof(hc), hipMemcpyDeviceToHost, ctx->stream));
  HIP_OK(hipStreamSynchronize(ctx->stream));
  for (int i = 0; i < 3; ++i) ctx->last_counters[i] = (int64_t)hc[i];
  ctx->last_counters[3] = (int64_t)T;
  if (o.w.hard && (rc = collect_hard_work(ctx, *o.w.hard))) return rc;
  if (sd && o.so.mu) ctx->soft_B = ctx->soft_N = -1;   // the slots' constants are no caller's state
  resolve_timings(ctx);
  return 0;
}

// ------------------------------------------------------------------ SQP driver
// sd (nullable): continuous batching -- d_x, d_u are the B slots of a stream of sd->P problems
// (tmpc_sqp_solve_stream_device); each problem's results go to its rows of sd's outputs
// keep_warm: the PCG warm-start buffer already holds this batch's starting lambdas (MPC loop)
int sqp_device(tmpc_ctx* ctx, int B, int N, double dt, int linsys, double* d_x, double* d_u, TraceDev* tr_out,
               bool keep_warm, bool hard_trace, const StreamDev* sd) {
  int rc = check_ready(ctx, B, N);
  if (rc) return rc;
  const int precond = precond_of(linsys);
  if (precond < 0)
    return fail(ctx, "linear system method %d is not available on the GPU (use S/PCG-J/BJ/SS = 1/2/3/4)", linsys);
  const int nj = ctx->hmodel.n, nx = 2 * nj;
  const ModelSel m = model_sel(ctx);
  const tmpc_options& o = ctx->opts;
  const std::vector<double> al = alpha_list(o);
  const int T = (int)al.size();
  const int W = o.max_iter_SQP_DDP + 1;
  Outer L{};
  if ((rc = outer_alloc(ctx, B, N, precond == 0, sd != nullptr, L))) return rc;
  Work& w = L.w;
  const ProbState& st = L.st;
  const AliveList& alv = L.alv;
  BUF(double, alphas, T + 1);
  BUF(double, terms, (size_t)B * T * N * 4);   // [B][T][N][cost, violation, D, soft value]
  BUF(unsigned long long, prob_counters, (size_t)B * 3);   // per-problem tallies of k_ls_decide
  const bool soft = L.soft;
  // UrdfCost has a state-dependent Hessian: it takes the per-knot Ghat path of the soft limits
  const bool perknot = soft || ctx->hcost.kind == COST_EE;
  if (perknot) {   // a stream's problems start from the initial constants
    if ((rc = init_soft(ctx, B, N, sd != nullptr, &w))) return rc;
    L.so.mu = ctx->soft_mu; L.so.lam = ctx->soft_lam; L.so.phi = ctx->soft_phi;
  }
  // hard box constraints (ACTIVE_SET / FULL_SET): per-knot rows, a banded Schur complement per problem
  HardArgs hard{};
  double* hterms = nullptr;
  const bool banded = qp_banded(ctx, N);
  if (banded) {
    if ((rc = setup_hard(ctx, B, N, T, precond, hard))) return rc;
    if (ctx->hlim.any_hard) hterms = hard.hterms;   // the limits' violation terms of the line search
    w.hard = &hard;
    w.Wtr = W;
    if (hard_trace && ctx->hlim.any_hard) {   // per-QP active-set bitmasks in the trace (tmpc_trace.hard_active)
      BUF(unsigned long long, tr_hard, (size_t)B * W * N);
      HIP_OK(hipMemsetAsync(tr_hard, 0, (size_t)B * W * N * sizeof(unsigned long long), ctx->stream));
      w.tr_active = tr_hard;
      L.tr.hard_active = tr_hard;
    }
  }
  if (o.pcg_warm_start && precond != 0 && banded)
    return fail(ctx, ctx->hlim.any_hard
                ? "pcg_warm_start with hard box constraints: the Schur dimension changes with the active set "
                  "from QP to QP, so a previous lambda is no PCG guess; unset pcg_warm_start"
                : "pcg_warm_start past the fused QP's rows: the banded PCG takes no guess; unset pcg_warm_start");
  if (o.pcg_warm_start && precond != 0) {
    // PCG warm start: each QP starts from the problem's previous lambda (in place: a workgroup reads
    // its guess before it writes its lambda)
    BUF(double, lam_warm, (size_t)B * N * nx);
    if (!keep_warm || sd) HIP_OK(hipMemsetAsync(lam_warm, 0, (size_t)B * N * nx * sizeof(double), ctx->stream));
    ctx->lam_warm = lam_warm;
    w.guess = lam_warm;
    w.lam_keep = lam_warm;
  }
  HIP_OK(hipMemsetAsync(L.counters, 0, 4 * sizeof(unsigned long long), ctx->stream));
  HIP_OK(hipMemsetAsync(prob_counters, 0, (size_t)B * 3 * sizeof(unsigned long long), ctx->stream));
  std::vector<double> al_h(al);
  al_h.push_back(0.0);  // slot T: alpha = 0 for the initial merit evaluation
  HIP_OK(hipMemcpyAsync(alphas, al_h.data(), al_h.size() * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
  if (sd) {   // slot s starts with problem s
    launch_stream_init(ctx->stream, B, *sd, d_x, d_u);
    HIP_OK(hipGetLastError());
  }
  // the goals of a tracking solve (a stream: of the problems now in the slots)
  if ((rc = goal_window(ctx, B, N, sd ? sd->period : B, sd ? "stream's period" : "batch size",
                        sd ? sd->slot_pid : nullptr, sd ? sd->pbase : 0, nullptr, &w.qp.gw)))
    return rc;
  bind_work(ctx, N, dt, d_x, d_u, st, w);
  // the line search's two launches: what the initial merit and an iteration's trials share
  LsTermsArgs lt{};
  lt.C = ctx->dcost; lt.Cs = ctx->dlim; lt.mu = L.so.mu; lt.lam = L.so.lam; lt.N = N; lt.dt = dt; lt.x = d_x; lt.u = d_u;
  lt.xs = w.xs; lt.terms = terms; lt.gw = w.qp.gw;
  DecideArgs ld{};
  ld.N = N; ld.NX = nx; ld.NU = nj; ld.soft = soft; ld.o = solver_opts(o); ld.terms = terms; ld.x = d_x; ld.u = d_u;
  ld.dx = w.qp.dx; ld.du = w.qp.du; ld.st = st; ld.tr = L.tr; ld.hterms = hterms;
  // initial J, c, merit (:541-548)
  auto init_merit = [&](int* mask, int* ac, int* activate) -> int {
    LsTermsArgs a = lt;
    a.P = alv.P; a.B = alv.nb; a.T = 1; a.alphas = alphas + T; a.active = mask;
    LAUNCH_OK(launch_ls_terms(val32(ctx), ctx->stream, m, a));
    if (hterms) LAUNCH_OK(hard_ls(ctx, nj, hard, B, N, 1, alphas + T, d_x, d_u, nullptr, nullptr, mask));
    DecideArgs d = ld;
    d.P = alv.P; d.B = alv.nb; d.T = 1; d.mode = LS_MODE_INIT; d.alphas = alphas + T; d.st.active = mask;
    d.active_count = ac; d.activate = activate;
    launch_ls_decide(ctx->stream, d);
    HIP_OK(hipGetLastError());
    return 0;
  };
  // one SQP iteration (:550-757)
  auto sqp_iteration = [&](int* ac) -> int {
    int rc2 = run_qp(ctx, B, precond, st, w, false, alv.P, alv.nb);
    if (rc2) return rc2;
    {
      LsTermsArgs a = lt;
      a.P = alv.P; a.B = alv.nb; a.T = T; a.alphas = alphas; a.dx = w.qp.dx; a.du = w.qp.du; a.active = st.active;
      Timed t(ctx, "ls_terms");
      LAUNCH_OK(launch_ls_terms(val32(ctx), ctx->stream, m, a));
      if (hterms) LAUNCH_OK(hard_ls(ctx, nj, hard, B, N, T, alphas, d_x, d_u, w.qp.dx, w.qp.du, st.active));
    }
    DecideArgs d = ld;
    d.P = alv.P; d.B = alv.nb; d.T = T; d.mode = LS_MODE_STEP; d.alphas = alphas; d.pcg_iters = w.qp.iters;
    d.active_count = ac; d.counters = prob_counters;
    if (w.hard && precond == 0) d.qp_singular = hard.sing;
    Timed t(ctx, "ls_decide");
    launch_ls_decide(ctx->stream, d);
    HIP_OK(hipGetLastError());
    return 0;
  };
  if ((rc = outer_run(ctx, B, N, L, d_x, d_u, sd, w.lam_keep, prob_counters, T, init_merit, sqp_iteration))) return rc;
  if (tr_out) *tr_out = L.tr;
  return 0;
}

// ------------------------------------------------------------------ iLQR driver (oracle/ilqr.py)
int ilqr_sweep_setup(tmpc_ctx* ctx, int B, int N, bool fresh_soft, IlqrSweep& q) {
  int rc = check_ready(ctx, B, N, false);
  if (rc) return rc;
  if (ctx->hcost.kind != COST_QUADRATIC) return fail(ctx, "iLQR supports QuadraticCost only (UrdfCost: use SQP)");
  if (ctx->hlim.any_hard)
    return fail(ctx, "iLQR has no constraint rows: hard box constraints (ACTIVE_SET / FULL_SET) need SQP");
  const int nj = ctx->hmodel.n, nx = 2 * nj, K = N - 1;
  const std::vector<double> al = alpha_list(ctx->opts);
  const int T = (int)al.size();
  BUF(double, alphas, T);
  BUF(double, il_K, (size_t)B * K * nj * nx);
  BUF(double, il_d, (size_t)B * K * nj);
  BUF(double, il_dV, (size_t)B * 2);
  BUF(int, il_ok, B);
  BUF(double, il_xt, (size_t)B * T * nx * N);
  BUF(double, il_ut, (size_t)B * T * nj * K);
  BUF(double, il_J, (size_t)B * T);
  q = IlqrSweep{};
  q.C = ctx->dcost; q.Cs = ctx->dlim; q.N = N;
  q.T = T; q.alphas = alphas; q.K = il_K; q.d = il_d; q.dV = il_dV; q.ok = il_ok; q.xt = il_xt; q.ut = il_ut;
  q.Jt = il_J;
  if (ctx->hlim.any) {
    if ((rc = init_soft(ctx, B, N, fresh_soft, nullptr))) return rc;
    q.mu = ctx->soft_mu;
    q.lam = ctx->soft_lam;
    BUF(double, il_jac_buf, (size_t)B * N * 3 * nj);   // soft-limit jacobians of every knot (Riccati sweep)
    q.jscratch = il_jac_buf;
  }
  HIP_OK(hipMemcpyAsync(alphas, al.data(), al.size() * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
  return 0;
}

int ilqr_sweeps(tmpc_ctx* ctx, const ProbState& st, const Work& w, PList P, int nb, const IlqrSweep& q) {
  if (int r = run_dynamics(ctx, w, P, nb)) return r;
  IlqrArgs a = q;   // the trajectory and the blocks the dynamics just wrote: as run_dynamics' (bind_work)
  a.P = P; a.B = nb; a.N = w.dyn.N; a.dt = w.dyn.dt; a.x = w.dyn.x; a.u = w.dyn.u; a.rho = st.rho; a.active = st.active;
  a.A = w.dyn.A; a.Bm = w.dyn.Bm; a.gw = w.qp.gw;
  { Timed t(ctx, "ilqr_backward"); LAUNCH_OK(launch_ilqr_backward(ric32(ctx), ctx->stream, ctx->hmodel.n, a)); }
  { Timed t(ctx, "ilqr_forward"); LAUNCH_OK(launch_ilqr_forward(val32(ctx), ctx->stream, model_sel(ctx), a)); }
  return 0;
}

int ilqr_device(tmpc_ctx* ctx, int B, int N, double dt, double* d_x, double* d_u, TraceDev* tr_out,
                const StreamDev* sd) {
  IlqrSweep q;
  int rc = ilqr_sweep_setup(ctx, B, N, sd != nullptr, q);   // a stream's problems start from the initial constants
  if (rc) return rc;
  const int nj = ctx->hmodel.n, nx = 2 * nj;
  const ModelSel m = model_sel(ctx);
  const int T = q.T;
  Outer L{};
  if ((rc = outer_alloc(ctx, B, N, false, sd != nullptr, L))) return rc;
  Work& w = L.w;
  const ProbState& st = L.st;
  const AliveList& alv = L.alv;
  BUF(unsigned long long, il_prob_counters, (size_t)B * 3);   // per-problem tallies of k_ilqr_decide
  HIP_OK(hipMemsetAsync(L.counters, 0, 4 * sizeof(unsigned long long), ctx->stream));
  HIP_OK(hipMemsetAsync(il_prob_counters, 0, (size_t)B * 3 * sizeof(unsigned long long), ctx->stream));
  if (q.mu) {   // the soft state the sweeps run on (ilqr_sweep_setup): the outer loop updates it
    L.so.mu = ctx->soft_mu; L.so.lam = ctx->soft_lam; L.so.phi = ctx->soft_phi;
  }
  StreamDev sdr{};
  if (sd) {
    // a stream's problems start from the rollout of u from x[:, 0] too: roll the `period` inputs out once
    // (the same kernel on the same x[:, 0], u as a batch solve's rollout, so the same trajectories) and
    // let the slots copy from there -- a pending problem then enters its slot without a serial rollout
    sdr = *sd;
    BUF(double, stream_xr, (size_t)sd->period * nx * N);
    HIP_OK(hipMemcpyAsync(stream_xr, sd->x_in, (size_t)sd->period * nx * N * sizeof(double), hipMemcpyDeviceToDevice,
                          ctx->stream));
    LAUNCH_OK(launch_rollout(val32(ctx), ctx->stream, m, Batch{{}, sd->period, N}, dt, stream_xr, sd->u_in));
    sdr.x_in = stream_xr;
    launch_stream_init(ctx->stream, B, sdr, d_x, d_u);   // slot s starts with problem s
    HIP_OK(hipGetLastError());
  } else {
    // iLQR iterates are rollouts: start from the rollout of u from x[:, 0]
    LAUNCH_OK(launch_rollout(val32(ctx), ctx->stream, m, Batch{{}, B, N}, dt, d_x, d_u));
  }
  // the goals of a tracking solve (a stream: of the problems now in the slots)
  if ((rc = goal_window(ctx, B, N, sd ? sd->period : B, sd ? "stream's period" : "batch size",
                        sd ? sd->slot_pid : nullptr, sd ? sd->pbase : 0, nullptr, &w.qp.gw)))
    return rc;
  bind_work(ctx, N, dt, d_x, d_u, st, w);
  // the decision's block: what the initial cost and an iteration share
  DecideArgs dc{};
  dc.N = N; dc.NX = nx; dc.NU = nj; dc.alphas = q.alphas; dc.o = solver_opts(ctx->opts); dc.Jt = q.Jt; dc.dV = q.dV;
  dc.ok = q.ok; dc.xt = q.xt; dc.ut = q.ut; dc.x = d_x; dc.u = d_u; dc.st = st; dc.tr = L.tr;
  // J at the current trajectory
  auto init_cost = [&](int* mask, int* ac, int* activate) -> int {
    IlqrArgs a = q;
    a.P = alv.P; a.B = alv.nb; a.x = d_x; a.u = d_u; a.active = mask; a.gw = w.qp.gw;
    LAUNCH_OK(launch_ilqr_init_cost(ctx->stream, nj, a));
    DecideArgs d = dc;
    d.P = alv.P; d.B = alv.nb; d.T = 1; d.init = 1; d.st.active = mask; d.active_count = ac; d.activate = activate;
    launch_ilqr_decide(ctx->stream, d);
    HIP_OK(hipGetLastError());
    return 0;
  };
  auto ilqr_iteration = [&](int* ac) -> int {
    if (int r = ilqr_sweeps(ctx, st, w, alv.P, alv.nb, q)) return r;
    DecideArgs d = dc;
    d.P = alv.P; d.B = alv.nb; d.T = T; d.active_count = ac; d.counters = il_prob_counters;
    Timed t(ctx, "ilqr_decide");
    launch_ilqr_decide(ctx->stream, d);
    HIP_OK(hipGetLastError());
    return 0;
  };
  // a stream's pending problems enter their slots from the rolled-out inputs; iLQR keeps no PCG warm start
  if ((rc = outer_run(ctx, B, N, L, d_x, d_u, sd ? &sdr : nullptr, nullptr, il_prob_counters, T, init_cost,
                      ilqr_iteration)))
    return rc;
  if (tr_out) *tr_out = L.tr;
  return 0;
}

// ------------------------------------------------------------------ continuous batching (include/tmpc.h, ABI 10)
// The stream's device descriptor and its B = min(slots, problems) slot buffers.
static int stream_setup(tmpc_ctx* ctx, int N, const tmpc_stream* s, StreamDev& sd, int& B, double** d_x,
                        double** d_u) {
  if (!s) return fail(ctx, "null stream");
  if (s->problems < 0 || s->slots < 1 || s->period < 1)
    return fail(ctx, "stream: problems %d (>= 0), slots %d and period %d (>= 1)", s->problems, s->slots, s->period);
  if (!s->x_in || !s->u_in) return fail(ctx, "stream: null x_in / u_in");
  if (s->trace.hard_active) return fail(ctx, "stream: trace.hard_active is not supported (set it to NULL)");
  if (s->substreams < 0 || s->substreams > 8) return fail(ctx, "stream: substreams %d (0..8)", s->substreams);
  B = std::min(s->slots, s->problems);
  const int nj = ctx->hmodel.n, nx = 2 * nj;
  BUF(double, stream_x, (size_t)std::max(B, 1) * nx * N);
  BUF(double, stream_u, (size_t)std::max(B, 1) * nj * (N - 1));
  BUF(int, stream_pid, std::max(B, 1));
  BUF(int, stream_next, 1);
  *d_x = stream_x;
  *d_u = stream_u;
  sd = StreamDev{};
  sd.P = s->problems; sd.pbase = 0; sd.period = s->period; sd.NX = nx; sd.NU = nj; sd.N = N;
  sd.W = ctx->opts.max_iter_SQP_DDP + 1; sd.MC = 6 * nj; sd.x_in = s->x_in; sd.u_in = s->u_in;
  sd.x_out = s->x_out; sd.u_out = s->u_out; sd.status = s->status;
  const tmpc_trace& t = s->trace;
  TraceDev& o = sd.tr_out;   // hard_active stays null
  o.iteration = t.iteration; o.ls_iter = t.line_search_iteration; o.alpha = t.alpha; o.rho = t.rho; o.J = t.J;
  o.c = t.c; o.merit = t.merit; o.D = t.D; o.ratio = t.reduction_ratio; o.accepted = t.succeeded_line_search;
  o.pcg_iters = t.pcg_iters; o.singular = t.singular;
  sd.slot_pid = stream_pid;
  sd.next = stream_next;
  return 0;
}

// One (sub-)stream on one context: problems [pbase, pbase + s->problems) of the caller's stream.
static int stream_one(tmpc_ctx* ctx, int N, double dt, int linsys, const tmpc_stream* s, int pbase) {
  StreamDev sd;
  int B = 0;
  double *d_x = nullptr, *d_u = nullptr;
  int rc = stream_setup(ctx, N, s, sd, B, &d_x, &d_u);
  if (rc || B == 0) return rc;
  sd.pbase = pbase;
  return linsys < 0 ? ilqr_device(ctx, B, N, dt, d_x, d_u, nullptr, &sd)
                    : sqp_device(ctx, B, N, dt, linsys, d_x, d_u, nullptr, false, false, &sd);
}

// The stream, split over K = substreams concurrent sub-streams: sub-stream c has its own context (HIP stream,
// buffers, lock-step loop on its own host thread), slots / K of the slots and a contiguous 1 / K of the
// problems.  Their kernels run side by side on the GPU, so one sub-stream's latency-bound phases (a one-wave
// Riccati sweep, a rollout with fewer lanes than SIMDs) overlap the other's.  Each problem's operations are
// unchanged, so its results are too.  linsys < 0: iLQR.
int stream_solve(tmpc_ctx* ctx, int N, double dt, int linsys, const tmpc_stream* s) {
  int rc = linsys < 0 ? check_ready(ctx, 1, N, false) : check_ready(ctx, 1, N);
  if (rc) return rc;
  if (!s) return fail(ctx, "null stream");
  ctx->mpc_last.B = 0;   // (sub-streams solve on contexts of their own: alloc_state of this one may not run)
  if (ctx->ref_R && ctx->hcost.kind == COST_EE)
    return fail(ctx, "a state reference (tmpc_set_reference) with UrdfCost: the task-space goal stays constant; "
                "clear the reference (tmpc_set_reference with R = 0)");
  if (ctx->ref_R > 1 && ctx->ref_R != s->period)
    return fail(ctx, "reference rows R = %d: must be 1 or the stream's period (%d)", ctx->ref_R, s->period);
  hipSetDevice(ctx->device);
  const int K = std::max(1, std::min({s->substreams, s->slots, std::max(1, s->problems), 8}));
  if (K == 1 || s->substreams <= 1) return stream_one(ctx, N, dt, linsys, s, 0);
  if (s->slots < 1 || s->problems < 0 || s->period < 1 || !s->x_in || !s->u_in)
    return stream_one(ctx, N, dt, linsys, s, 0);   // the argument errors, as for one stream
  while ((int)ctx->subs.size() < K) {
    tmpc_ctx* sub = nullptr;
    if (tmpc_create(ctx->device, &sub) != 0) return fail(ctx, "stream: creating sub-stream context failed");
    ctx->subs.push_back(sub);
  }
  for (int c = 0; c < K; ++c) {   // the configuration of this context
    tmpc_ctx* sub = ctx->subs[c];
    sub->hmodel = ctx->hmodel;
    sub->hcost = ctx->hcost;
    sub->hlim = ctx->hlim;
    sub->model_id = ctx->model_id;
    sub->opts = ctx->opts;
    sub->has_model = ctx->has_model;
    sub->has_cost = ctx->has_cost;
    sub->ref_dev = ctx->ref_dev;   // borrowed: read-only, and this call outlives the sub-streams' solves
    sub->ref_R = ctx->ref_R;
    sub->ref_M = ctx->ref_M;
    sub->ref_step = 0;
    sub->soft_B = sub->soft_N = -1;
    sub->stats.clear();
    sub->kbytes.clear();
    sub->err.clear();
    HIP_OK(hipMemcpyAsync(sub->dmodel, &sub->hmodel, sizeof(ModelDev), hipMemcpyHostToDevice, sub->stream));
    HIP_OK(hipMemcpyAsync(sub->dcost, &sub->hcost, sizeof(CostDev), hipMemcpyHostToDevice, sub->stream));
    HIP_OK(hipMemcpyAsync(sub->dlim, &sub->hlim, sizeof(ConstrDev), hipMemcpyHostToDevice, sub->stream));
    HIP_OK(hipStreamSynchronize(sub->stream));
  }
  std::vector<tmpc_stream> part(K, *s);
  std::vector<int> pbase(K, 0), rcs(K, 0);
  for (int c = 0, p0 = 0; c < K; ++c) {
    part[c].problems = s->problems / K + (c < s->problems % K ? 1 : 0);
    part[c].slots = s->slots / K + (c < s->slots % K ? 1 : 0);
    part[c].substreams = 1;
    pbase[c] = p0;
    p0 += part[c].problems;
  }
  std::vector<std::thread> th;
  for (int c = 0; c < K; ++c)
    th.emplace_back([&, c]() {
      hipSetDevice(ctx->device);
      rcs[c] = stream_one(ctx->subs[c], N, dt, linsys, &part[c], pbase[c]);
    });
  for (auto& t : th) t.join();
  for (int c = 0; c < K; ++c)
    if (rcs[c]) return fail(ctx, "sub-stream %d: %s", c, ctx->subs[c]->err.c_str());
  for (int i = 0; i < 3; ++i) {
    ctx->last_counters[i] = 0;
    for (int c = 0; c < K; ++c) ctx->last_counters[i] += ctx->subs[c]->last_counters[i];
  }
  ctx->last_counters[3] = ctx->subs[0]->last_counters[3];
  for (int c = 0; c < K; ++c) {   // kernel timings and counted bytes of every sub-stream
    for (auto& kv : ctx->subs[c]->stats) {
      ctx->stats[kv.first].launches += kv.second.launches;
      ctx->stats[kv.first].total_ms += kv.second.total_ms;
    }
    for (auto& kv : ctx->subs[c]->kbytes) ctx->kbytes[kv.first] += kv.second;
  }
  ctx->soft_B = ctx->soft_N = -1;
  return 0;
}

// ------------------------------------------------------------------ receding-horizon MPC (oracle/mpc.py)
// what the MPC loop and its single step refuse
static int mpc_ready(tmpc_ctx* ctx, int B, int N, int solver) {
  const bool ilqr = solver == TMPC_SOLVER_ILQR;
  int rc = check_ready(ctx, B, N, !ilqr);
  if (rc) return rc;
  if (ctx->hmodel.n > NJ_FULL)
    return fail(ctx, "the MPC loop supports up to %d joints (got %d)", NJ_FULL, ctx->hmodel.n);
  if (ctx->hcost.kind != COST_QUADRATIC) return fail(ctx, "the MPC loop supports QuadraticCost only");
  if (!ilqr && precond_of(solver) < 0) return fail(ctx, "solver %d: use TMPC_LINSYS_* or TMPC_SOLVER_ILQR", solver);
  if (!ilqr && ctx->opts.pcg_warm_start && precond_of(solver) != 0 && qp_banded(ctx, N))
    return fail(ctx, "pcg_warm_start with hard box constraints or past the fused QP's rows: the banded PCG takes "
                "no guess; unset pcg_warm_start");
  return 0;
}

// where one step's outputs go (AdvanceArgs: first element and row stride of each; all nullable)
struct MpcStepOut {
  double* x_next; size_t x_ld;
  double* u0; size_t u_ld;
  int *code, *iters; size_t st_ld;
};

// One iteration of oracle/mpc.py's loop on the stream: the horizon solve of step `step`, then everything between
// two solves in one launch (k_mpc_advance: the plant step and the status into `out`, the shifts of x, u, the warm
// lambda and the soft constants) and QF_start one down.  No synchronisation of its own beyond the solve's.
static int mpc_one_step(tmpc_ctx* ctx, int B, int N, double dt, int solver, int step, double* d_x, double* d_u,
                        const MpcStepOut& out) {
  const bool ilqr = solver == TMPC_SOLVER_ILQR;
  ctx->ref_step = step;   // a reference slides one column per step (goal_window)
  int rc = ilqr ? ilqr_device(ctx, B, N, dt, d_x, d_u, nullptr)
                : sqp_device(ctx, B, N, dt, solver, d_x, d_u, nullptr, /*keep_warm=*/step > 0);
  ctx->ref_step = 0;
  if (rc) return rc;
  {
    Timed t(ctx, "mpc_shift");
    AdvanceArgs a{};
    a.B = B; a.N = N; a.dt = dt; a.x = d_x; a.u = d_u;
    a.x_out = out.x_next; a.x_ld = out.x_ld; a.u_out = out.u0; a.u_ld = out.u_ld;
    a.code_out = out.code; a.iter_out = out.iters; a.st_ld = out.st_ld;
    a.exit_code = ctx->last_st.exit_sqp; a.iter = ctx->last_st.iter;
    // the next step's first PCG starts from this step's last lambda shifted by one knot (oracle/mpc.py)
    if (!ilqr && ctx->opts.pcg_warm_start && precond_of(solver) != 0 && !qp_banded(ctx, N)) a.lam_warm = ctx->lam_warm;
    if (ctx->hlim.any) { a.Cs = ctx->dlim; a.mu = ctx->soft_mu; a.lam = ctx->soft_lam; a.phi = ctx->soft_phi; }
    LAUNCH_OK(launch_mpc_advance(ctx->stream, model_sel(ctx), a));
  }
  // QuadraticCost.shift_QF_start(-1) (TrajoptCost.py:100-104)
  if (ctx->hcost.QF_start >= 0) {
    ctx->hcost.QF_start = ctx->hcost.QF_start > 0 ? ctx->hcost.QF_start - 1 : 0;
    HIP_OK(hipMemcpyAsync(ctx->dcost, &ctx->hcost, sizeof(CostDev), hipMemcpyHostToDevice, ctx->stream));
  }
  return 0;
}

int mpc_device(tmpc_ctx* ctx, int B, int N, double dt, int solver, int steps, double* d_x, double* d_u,
               double* d_xe, double* d_ue, int* d_codes, int* d_iters) {
  int rc = mpc_ready(ctx, B, N, solver);
  if (rc) return rc;
  if (steps < 1) return fail(ctx, "steps must be >= 1");
  const int nx = 2 * ctx->hmodel.n;
  // work counters of the whole loop: the sum over its horizon solves (tmpc_solve_counters)
  int64_t sum_counters[3] = {0, 0, 0};
  // executed state 0 = x[:, 0]
  HIP_OK(hipMemcpy2DAsync(d_xe, (size_t)(steps + 1) * sizeof(double), d_x, (size_t)N * sizeof(double), sizeof(double),
                          (size_t)B * nx, hipMemcpyDeviceToDevice, ctx->stream));
  auto col = [](auto* p, int c) { return p ? p + c : p; };   // (a null output stays null)
  for (int s = 0; s < steps; ++s) {   // step s fills column s + 1 of x_exec and column s of u_exec, codes, iters
    const size_t ld = (size_t)steps;
    rc = mpc_one_step(ctx, B, N, dt, solver, s, d_x, d_u,
                      {d_xe + s + 1, ld + 1, col(d_ue, s), ld, col(d_codes, s), col(d_iters, s), ld});
    if (rc) return rc;
    for (int i = 0; i < 3; ++i) sum_counters[i] += ctx->last_counters[i];
  }
  HIP_OK(hipStreamSynchronize(ctx->stream));
  for (int i = 0; i < 3; ++i) ctx->last_counters[i] = sum_counters[i];
  return 0;
}

// One step of the loop above for a caller that closes the loop itself (include/tmpc.h tmpc_mpc_step_device): the
// measured state into x[:, 0], then the loop's step.
int mpc_step_device(tmpc_ctx* ctx, int B, int N, double dt, int solver, int step, double* d_x, double* d_u,
                    const tmpc_mpc_io& io) {
  int rc = mpc_ready(ctx, B, N, solver);
  if (rc) return rc;
  if (!d_x || !d_u) return fail(ctx, "null x/u");
  if (step < 0) return fail(ctx, "step must be >= 0 (got %d)", step);
  if (step > 0) {
    // the warm lambda, the soft constants and QF_start on the device are the previous solve's: they continue
    // this loop only if that solve was the loop's previous step
    const auto& l = ctx->mpc_last;
    if (l.B == 0)
      return fail(ctx, "MPC step %d: the context's previous solve was not an MPC step (a fresh context, or another "
                  "solve, stream or configuration change since); expected step 0, which starts a loop", step);
    if (l.B != B || l.N != N || l.dt != dt || l.solver != solver || l.step != step - 1)
      return fail(ctx, "MPC step %d (B=%d, N=%d, dt=%g, solver=%d): the context's previous solve was step %d of "
                  "B=%d, N=%d, dt=%g, solver=%d; expected step %d of that loop, or step 0 to start a new one",
                  step, B, N, dt, solver, l.step, l.B, l.N, l.dt, l.solver, l.step + 1);
  }
  const int nx = 2 * ctx->hmodel.n;
  if (io.x_meas)   // x[:, 0] <- x_meas, on the stream
    HIP_OK(hipMemcpy2DAsync(d_x, (size_t)N * sizeof(double), io.x_meas, sizeof(double), sizeof(double), (size_t)B * nx,
                            hipMemcpyDeviceToDevice, ctx->stream));
  rc = mpc_one_step(ctx, B, N, dt, solver, step, d_x, d_u,
                    {io.x_pred, 1, io.u0, 1, io.status, io.status ? io.status + 1 : nullptr, 2});
  if (rc) return rc;
  HIP_OK(hipStreamSynchronize(ctx->stream));   // the caller reads u0 next
  ctx->mpc_last = {B, N, solver, step, dt};
  return 0;
}

}  // namespace tmpc
