// Internal declarations shared by the kernels (the QP side in tmpc_kernels.hip and tmpc_qp.hip, the solve loops' state
// machine in tmpc_state.hip, ...) and the C-ABI / solver driver (tmpc_api.cpp).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>

#include "tmpc_device.h"
#include "tmpc_models.h"
#include "tmpc_state.h"   // SolverOpts and the state machine's scalar rules

struct tmpc_ctx;

namespace tmpc {

// context accessors for the other translation units (tmpc_comm.cpp)
int ctx_fail(tmpc_ctx* ctx, const char* fmt, ...);
int ctx_device(const tmpc_ctx* ctx);
hipStream_t ctx_stream(const tmpc_ctx* ctx);

// The problems a batch-iteration launch visits: launches over B problems take (PList, nb) and visit
// problems P.at(p) for p < nb (and p < *P.cnt).  idx null: the identity, nb = B.  Otherwise idx is the
// ascending list of the problems still alive in the lock-step loop (k_alive_list, rebuilt at the end of
// every batch iteration on the stream, so exact when a launch reads it) and nb the host's upper bound
// of its length (the count of two iterations before: aliveness only ever ends).  Every kernel still
// tests its own per-problem mask (active / need_grad / ...): the list only drops the problems that can
// no longer be active, so the lock-step tail stops dispatching thousands of early-exit workgroups.
struct PList {
  const int* idx;
  const int* cnt;
  __device__ __forceinline__ int at(int p) const { return idx ? idx[p] : p; }
  __device__ __forceinline__ bool has(int p, int nb) const { return p < nb && (!cnt || p < *cnt); }
};
void launch_alive_list(hipStream_t s, int B, const int* alive, int* idx, int* cnt, int* host_slot = nullptr);

// PRECOND_NONE: the identity preconditioner '0' (PCG.py:114-118)
enum { PRECOND_J = 1, PRECOND_BJ = 2, PRECOND_SS = 3, PRECOND_NONE = 4 };
enum { LS_MODE_INIT = 0, LS_MODE_STEP = 1 };
// QP_MODE_*: tmpc_dispatch.h

// per-problem solver state (device arrays, SoA)
struct ProbState {
  double* rho;
  double* drho;
  double* J;
  double* c;
  double* merit;
  int* iter;
  int* active;
  int* need_grad;
  int* exit_sqp;
};

// per-problem trace rows [B][max_iter_sqp + 1] (self.trace, :555-569, :691-743)
struct TraceDev {
  int* iteration;
  int* ls_iter;
  double* alpha;
  double* rho;
  double* J;
  double* c;
  double* merit;
  double* D;
  double* ratio;
  int* accepted;
  int* pcg_iters;
  int* singular;                  // the QP took the least-squares answer (reference: self.singular)
  unsigned long long* hard_active;   // [B][W][N] per-knot active-set bitmasks of the QP (nullable)
};

// the model a launch runs on (tmpc_ctx.h model_sel); mid 0: the runtime model, whose coefficients M holds
struct ModelSel { int nj; bool chain; int mid; const ModelDev* M; };
// the problems a launch visits (PList above, B its bound) and the horizon
struct Batch { PList P; int B, N; };

// The launchers' argument blocks: a caller value-initialises one (`Args a{};`: pointers null, the PList the
// identity), fills it by name and passes it by const&.  A field is named as the kernel parameter it feeds.
// f32: the dynamics (launch_ilqr_backward: the Riccati sweep) in fp32, tmpc_options.precision; buffers stay fp64

// the dynamics of the problems that need fresh gradients (run_dynamics' three launches)
struct DynArgs : Batch {
  double dt;
  const double *x, *u, *xs;
  const int* need;
  // launch_qp_fd: qdd (where the gradient is taken), the defects cvec; launch_qp_minv: minv; launch_qp_grad: A, Bm
  double *qdd, *cvec, *minv, *A, *Bm;
  // the unit entry points (launch_unit_*: tmpc_fd_batch, tmpc_fd_grad_batch) read K states x [K][nx], u [K][nu] in
  // place of the Batch, xs, need and cvec; launch_unit_fd writes qdd and xnext (nullable), launch_unit_grad dqdd too
  int K;
  double *xnext, *dqdd;
};
int launch_qp_fd(bool f32, hipStream_t s, const ModelSel& m, const DynArgs& a);
int launch_qp_minv(bool f32, hipStream_t s, const ModelSel& m, const DynArgs& a);
int launch_qp_grad(bool f32, hipStream_t s, const ModelSel& m, const DynArgs& a);
// the line search's per-knot merit terms [B][T][N][4] of the T trials x - alphas[t] dx, u - alphas[t] du
struct LsTermsArgs : Batch {
  const CostDev* C;
  const ConstrDev* Cs;
  const double *mu, *lam;   // the soft limits' state (null: none)
  int T;
  double dt;
  const double *alphas, *x, *u, *xs;
  const double *dx, *du;    // null: the terms at x, u themselves (the initial merit)
  const int* active;
  double* terms;
  const double* gw;         // the goal window of a tracking solve (below), else null
};
int launch_ls_terms(bool f32, hipStream_t s, const ModelSel& m, const LsTermsArgs& a);
// The goal window (tmpc_set_reference): gw [B][N][nx], knot-major -- the state goal of problem b's knot k, which
// the tracking instances of the goal-reading kernels (their TRK template argument) read in place of CostDev::xg.
// A null gw launches the fixed-goal instances, which are the kernels as they were.  launch_goal_window resolves
// the reference xref [R][nx][M] for one horizon solve: gw[b][k] = xref[(pbase + (pid ? pid[b] : b)) % R]
// [:, min(k + step, M - 1)], for the problems in `mask` (null: all; a stream's slot with pid < 0 is skipped).
struct GoalWindowArgs {
  int B, N, nx, R, M, step, pbase;
  const double* xref;
  const int *pid, *mask;
  double* gw;
};
void launch_goal_window(hipStream_t s, const GoalWindowArgs& a);
// (the launchers of the tracking instances, which live in translation units of their own: tmpc_fd_trk.hip,
// tmpc_ilqr_trk.hip; launch_ls_terms / launch_ilqr_* call them when gw is set)
int launch_ls_terms_trk(bool f32, hipStream_t s, const ModelSel& m, const LsTermsArgs& a);
int launch_unit_fd(bool f32, hipStream_t s, const ModelSel& m, const DynArgs& a);
int launch_unit_minv(bool f32, hipStream_t s, const ModelSel& m, const DynArgs& a);
int launch_unit_grad(bool f32, hipStream_t s, const ModelSel& m, const DynArgs& a);
// b / mask: the problems to roll out (the identity and every problem by default; the stream's refilled
// slots: the alive list and act_init)
int launch_rollout(bool f32, hipStream_t s, const ModelSel& m, const Batch& b, double dt, double* x, const double* u,
                   const int* mask = nullptr);
int launch_ginv(hipStream_t s, int nj, const CostDev* C, PList P, int B, const double* rho, const int* active, double* G);
// The QP family's block, grouped by the launchers that read a field.  launch_qp (k_qp): mode SCHUR writes Sd / Sl /
// gam, DXU reads lam and writes dx / du, PCG does all three around its PCG (outputs Sd, Sl, gam, Pd nullable).
struct QpArgs : Batch {
  // every launcher: the Schur system S lam = gam (launch_btsolve: of every problem b < B, it takes no problem list)
  double *Sd, *Sl, *gam, *lam;
  // launch_qp, launch_qp_blocks, launch_pcg
  int precond;
  double tol;
  int max_iter;
  const double* guess;     // PCG initial iterate [B][N nx] (nullable)
  int* iters;
  // launch_qp, launch_qp_blocks
  int mode;
  const double* G;         // (Q + rho I)^-1 blocks [B][3][nx nx] (k_ginv); with jsoft the per-knot Gk (k_ginv_soft)
  const double *A, *Bm, *cvec;
  double *dx, *du;
  // launch_qp only
  const CostDev* C;
  bool cost_diag;          // C is a QuadraticCost with CostDev.diag set (the host's copy; picks the PcgRowC instances)
  double dt;      // the Euler step of A_k / B_k (their structural rows are not read, tmpc_qp.hip qp_schur_row)
  const double *x, *u;
  const int* active;       // launch_btsolve too
  const double* jsoft;     // soft limits: the knots' jacobian terms (else null)
  double* Sg;              // S / P^-1 rows in HBM scratch (the GM instances below), else null
  const double* gw;
  double* Pd;              // launch_pcg too: the preconditioner's diagonal blocks (nullable)
  // launch_qp_blocks only (the plugin-hook QP on caller-formed blocks, tmpc_hooks.hip): G holds full
  // (G_k + rho I)^-1 blocks with launch_ghat_full's per-problem pivot flags err, cvec the caller's c, g its gradient
  const double* g;
  const int* err;
  // launch_pcg only (the stand-alone PCG, tmpc_pcg_batch): the upper blocks (null: Sl's transposes), iteration traces
  const double* Su;
  double *tnu, *tres;
  // launch_btsolve only (method S: the direct block-tridiagonal solve): scratch
  double *U, *Y;
};
int launch_qp(hipStream_t s, int nj, const QpArgs& a);
// largest Schur dimension N nx of the fused QP: up to 1024 rows S / P^-1 stay in registers, up to
// QP_MAX_ROWS (the GM kernels: two rows per lane, 12 waves = 3 per SIMD, i.e. 168 VGPRs) in HBM
// scratch Sg of qp_gm_doubles(B, N, nx) doubles.  1536 = arm6 at N = 128 (BASELINE config 5).
constexpr int QP_MAX_ROWS = 1536;
inline size_t qp_gm_doubles(int B, int N, int nx) { return (size_t)B * 4 * nx * (size_t)N * nx; }
// rows from which the QP takes the GM kernel: 1025, or TMPC_QP_GM_MIN_ROWS (parity tests run the GM
// kernel on the reference's N = 64 fixtures this way)
inline int qp_gm_min_rows() {
  const char* e = getenv("TMPC_QP_GM_MIN_ROWS");
  const int v = e ? atoi(e) : 0;
  return v > 0 ? v : 1025;
}
// soft limits: the per-knot Ghat blocks and jacobian terms of the QP, at the soft state mu / lam
struct GinvSoftArgs : Batch {
  const CostDev* C;
  const ConstrDev* Cs;
  const double* rho;
  const int* active;
  const double *x, *u, *mu, *lam;
  double *Gk, *jsoft;
};
int launch_ginv_soft(hipStream_t s, int nj, const GinvSoftArgs& a);
int launch_pcg(hipStream_t s, int nx, const QpArgs& a);
// plugin-hook QP on caller-formed blocks (tmpc_hooks.hip)
int launch_ghat_full(hipStream_t s, int nj, int B, int N, const double* G, const double* rho, double* Gh, int* err);
int launch_qp_blocks(hipStream_t s, int nj, const QpArgs& a);
int qp_blocks_set_max_lds();
int launch_btsolve(hipStream_t s, int nx, const QpArgs& a);
int pcg_set_max_lds();
void launch_sum_counters(hipStream_t s, int B, const unsigned long long* pc, unsigned long long* out);
// Continuous batching (tmpc_sqp_solve_stream_device / tmpc_ilqr_solve_stream_device): B resident slots
// work through a stream of P problems.  The workgroup of k_soft_outer that ends a problem's outer loop
// (outer_active 1 -> 0) writes the problem's results to its output rows and, when a problem is pending
// (one atomic on `next`; which slot gets which problem changes no problem's results), loads the next
// one's inputs with the state a fresh solve starts from -- act_init, so its initial merit / cost is
// evaluated in the same batch iteration.  Each problem's own operation sequence is the one of a batch
// solve, so its results are bitwise those of tmpc_*_solve_batch.
struct StreamDev {
  int P, period, NX, NU, N, W, MC;   // problems, input period, sizes, trace rows, soft slots per knot (6 n)
  int pbase;                         // global index of this (sub-)stream's problem 0 (inputs and output rows)
  const double* x_in;                // [period][NX][N]: problem p starts from input (pbase + p) % period
  const double* u_in;                // [period][NU][N-1]
  double* x_out;                     // [pbase + P][NX][N] (nullable): problem p's row is pbase + p
  double* u_out;                     // [pbase + P][NU][N-1] (nullable)
  int* status;                       // [pbase + P][4]: exit code, iterations, exit_soft, outer_iter (nullable)
  TraceDev tr_out;                   // [pbase + P][W] per field (each nullable; hard_active unused)
  int* slot_pid;                     // [B] problem in the slot (-1: none)
  int* next;                         // [1] next pending problem
};
void launch_stream_init(hipStream_t s, int B, const StreamDev& sd, double* x, double* u);

// the decision that ends an iteration: a trial into x, u, the problem's state and trace, the count of live problems
struct DecideArgs : Batch {
  int NX, NU, T;
  const double* alphas;
  SolverOpts o;
  double *x, *u;
  ProbState st;
  TraceDev tr;
  int* active_count;
  unsigned long long* counters;   // [B][3] per-problem tallies (iterations, -, fresh gradients): launch_sum_counters
  int* activate;   // initial merit / cost only, nullable: the real active flags -- st.active is then the act_init
                   // mask, cleared as the problem enters its inner loop
  // launch_ls_decide
  int mode, soft;
  const double *terms, *dx, *du;
  const int* pcg_iters;
  const double* hterms;     // hard limits: the violation terms of launch_hard_ls (else null)
  const int* qp_singular;   // HardArgs.sing of the direct banded solve (else null)
  // launch_ilqr_decide
  int init;
  const double *Jt, *dV, *xt, *ut;
  const int* ok;
};
void launch_ls_decide(hipStream_t s, const DecideArgs& a);

// outer_active (nullable): only the problems still in their outer loop
void launch_init_state(hipStream_t s, int B, double rho_init, const ProbState& st,
                       const int* outer_active = nullptr);
struct SoftOuterArgs : Batch {
  const ConstrDev* Cs;
  int nj;
  double tol;
  int max_iter;
  double *x, *u, *mu, *lam, *phi;
  int *outer_active, *outer_iter, *exit_soft, *outer_count;
  // the per-problem outer loop (null act_init: lock-step, tmpc_state.hip)
  ProbState st;
  int* act_init;
  double rho_init;
  // a stream's hand-over of finished slots (sd.P = 0: none; per-problem mode only)
  StreamDev sd;
  double* xs;
  TraceDev tr;
  double* lam_warm;
};
void launch_soft_outer(hipStream_t s, const SoftOuterArgs& a);

// One iLQR iteration's sweeps: what the backward sweep leaves for the forward one and the T trials' rollouts and
// costs for the decision.  Trials are knot-major ([B][T][N][nx], [B][T][N-1][nu]: tmpc_ilqr.hip).
struct IlqrArgs : Batch {
  const CostDev* C;
  const ConstrDev* Cs;
  const double *mu, *lam;      // the soft limits' state the sweeps run on (null: none)
  int T;                       // line-search trials, alpha_list of the options
  double dt;
  int init;                    // launch_ilqr_forward: the cost of x, u themselves (no feedback law, T = 1)
  const double* alphas;        // [T]
  const double *x, *u, *rho;
  const int* active;           // launch_ilqr_init_cost: its mask
  const double *A, *Bm;
  double* jscratch;            // soft limits: the knots' jacobians [B][N][3 n] (else null)
  double *K, *d, *dV;          // [B][N-1][nu][nx], [B][N-1][nu], [B][2]
  int* ok;                     // [B]
  double *xt, *ut, *Jt;        // [B][T][N][nx], [B][T][N-1][nu], [B][T]
  const double* gw;
};
int launch_ilqr_backward(bool f32, hipStream_t s, int nj, const IlqrArgs& a);
int launch_ilqr_forward(bool f32, hipStream_t s, const ModelSel& m, const IlqrArgs& a);
int launch_ilqr_init_cost(hipStream_t s, int nj, const IlqrArgs& a);
int launch_ilqr_backward_trk(bool f32, hipStream_t s, int nj, const IlqrArgs& a);
int launch_ilqr_forward_trk(bool f32, hipStream_t s, const ModelSel& m, const IlqrArgs& a);
int launch_ilqr_init_cost_trk(hipStream_t s, int nj, const IlqrArgs& a);

void launch_ilqr_decide(hipStream_t s, const DecideArgs& a);
// BoxConstraint.__init__ (:21-24) for a slot of soft type t: mu = mu_init, lambda = 0, phi = phi_init
struct SoftInit { double mu, lam, phi; };
__device__ __forceinline__ SoftInit soft_initial(const ConstrDev* __restrict__ Cs, int t) {
  return {Cs->mu_init[t], 0.0, Cs->phi_init[t]};
}

// Everything between two horizon solves of the MPC loop (oracle/mpc.py), in one launch per step:
//   * the plant: x_next = x_0 + dt * (qd_0, qdd(x_0, u_0)), nominal explicit Euler in fp64 (TrajoptPlant.py:92-99),
//     each component one __dmul_rn and one __dadd_rn; x_next and u_0 go to x_out / u_out, the solve's exit code
//     and iteration count to code_out / iter_out;
//   * the trajectory shifted by one knot: x_k <- x_{k+1}, u_k <- u_{k+1}, last knot kept, x_0 <- x_next;
//   * the PCG warm start lam_warm [B][N][nx] shifted by one block, last block kept;
//   * the soft constants mu / lam / phi [B][N][6 nj] as BoxConstraint.shift_soft_constraint_constants(1) shifts
//     them (TrajoptConstraint.py:168-176): arr[:, :-1] = arr[:, 1:]; arr[:, 1:] = init -- knot 0 takes knot 1's
//     value and every later knot of the slot's span returns to soft_initial; torque rows span N - 1 knots.
// An output row is (problem, component) for the doubles and the problem for the ints; *_ld is the element stride
// between consecutive rows, so one kernel writes a step's own arrays (tmpc_mpc_step_device: ld 1, status ld 2)
// and a column of the loop's (tmpc_mpc_batch: x_exec [B][nx][steps + 1], u_exec [B][nu][steps], codes / iters
// [B][steps]).  x_out, u_out, code_out, iter_out, lam_warm and mu (with lam, phi, Cs) are nullable.
struct AdvanceArgs {
  int B, N;
  double dt;
  double *x, *u;
  double* x_out; size_t x_ld;
  double* u_out; size_t u_ld;
  int *code_out, *iter_out; size_t st_ld;
  const int *exit_code, *iter;   // the solve's per-problem state (ProbState), read when code_out / iter_out is set
  double* lam_warm;
  const ConstrDev* Cs;
  double *mu, *lam, *phi;
};
int launch_mpc_advance(hipStream_t s, const ModelSel& m, const AdvanceArgs& a);

void launch_outer_init(hipStream_t s, int B, int* outer_active, int* outer_iter, int* exit_soft);
void launch_soft_init(hipStream_t s, const ConstrDev* Cs, size_t total, int MC, double* mu, double* lam,
                      double* phi);

// The banded QP (tmpc_hard.hip: hard box constraints, the QP past QP_MAX_ROWS rows, the plugin-hook QP's banded
// path): one block for its launchers, grouped by the launchers that read a field.
struct HardArgs {
  // every launcher
  int B, N;
  const int* active;
  // launch_hard_schur, launch_hard_solve, launch_hard_dxu: the knots' rows, the row layout, S lam = gam
  int rmax, dmax, W;              // rows per knot and Schur rows at most; the band's half-width
  int *cnt, *hcol;                // [B][N] rows of each knot; [B][N][rmax] each row's column of [x_k; u_k]
  int *roff, *hoff, *dim;         // [B][N] first row of R_j, of H_k; [B] the Schur dimension (launch_hard_schur writes)
  double *hsgn, *Sb, *gam, *lam;  // [B][N][rmax] the rows' signs; [B][2W+1][dmax] row-start-relative band; [B][dmax] each
  int* rng;                       // [B][dmax][2] first / last structurally nonzero column of each row of S
  // launch_hard_schur, launch_hard_dxu (launch_hard_track_grad: C, x, u, jsoft; launch_hard_ls: x, u)
  const CostDev* C;
  const double *x, *u, *Ghat, *A, *Bm, *jsoft;
  int per_knot;                   // Ghat: 0 [B][3][nx nx] (k_ginv), 1 per knot (soft limits, k_ginv_soft), 2 below
  // the plugin-hook QP (tmpc_qp_blocks_banded_batch): per_knot = 2 -- Ghat holds full (G_k + rho I)^-1 blocks
  // [B][N][nx+nu][nx+nu] -- the caller's cost gradient gvec [B][N][nx+nu] (null: the context's cost), and
  // rows_given: cnt / hcol / hsgn / hval were filled from the caller's constraint hooks (k_hard_rows skipped)
  const double* gvec;
  int rows_given;
  // launch_hard_schur only
  const ConstrDev* Cs;            // launch_hard_ls too
  const double* cvec;
  double *hval, *Y;               // [B][N][rmax] the rows' values; scratch [B][2][nx+nu][dmax], Ghat times the rows' pieces
  int *rkind, *rknot, *ridx;      // [B][dmax] per row: dynamics / hard, knot, index (k_hard_layout)
  int* hslot;                     // [B][N][rmax] t * 2n + e of each row
  unsigned long long* amask;      // [B][N] active-set bitmask per knot (bit t * 2n + e)
  const int* iter;                // per-problem SQP iteration (trace row iter + 1)
  int Wtr;                        // trace row stride (max_iter_SQP_DDP + 1)
  unsigned long long* tr_active;  // [B][Wtr][N] trace copy of amask (nullable)
  // launch_hard_solve only: precond 0 the banded elimination (M, rhs, sing), else the PCG
  int precond, max_iter;
  double tol;
  int* iters;
  double *Pd, *Pl, *Ptr, *M, *rhs;   // the PCG's preconditioner blocks past its LDS cache; the elimination's S and gam
  double* work;                   // [B] algorithmic HBM bytes of k_hard_pcg, accumulated per problem (nullable)
  int* sing;                      // [B] the direct solve took the least-squares answer (singular S)
  // launch_hard_dxu (writes), launch_hard_ls (reads: the trial points x - alpha dx, u - alpha du; null: x, u)
  double *dx, *du;
  // launch_hard_ls only
  int T;
  const double* alphas;           // [T]
  double* hterms;                 // [B][T][N]
};
// k_hard_pcg: 1024 threads per problem, row a on thread a % 1024 (row slot a / 1024, at most 4 slots)
constexpr int HARD_PCG_THREADS = 1024, HARD_PCG_MAX_SLOTS = 4;
constexpr int HARD_PCG_MAX_ROWS = HARD_PCG_THREADS * HARD_PCG_MAX_SLOTS;
constexpr int HARD_PCG_LDS_BYTES = 160 * 1024;   // all of a CU's LDS: vectors + preconditioner-block cache
int launch_hard_schur(hipStream_t s, int nj, const HardArgs& h);
int launch_hard_solve(hipStream_t s, int nj, const HardArgs& h);
int launch_hard_dxu(hipStream_t s, int nj, const HardArgs& h);
int launch_hard_ls(hipStream_t s, int nj, const HardArgs& h);
// the banded QP's cost gradient against the goal window gw (hard_grad's expressions with gw[b][k] for xg), into
// gvec [B][N][nx+nu]: HardArgs.gvec of a tracking solve, so k_hard_schur / k_hard_dxu run unchanged
int launch_hard_track_grad(hipStream_t s, int nj, const HardArgs& h, const double* gw, double* gvec);
// dynamic LDS of k_hard_schur (one workgroup per problem): the cost gradient / piece record per knot
// (3 nj doubles + 2 ints), the rows' piece knots (2 dmax ints, 16-byte rounded) and the shared Ghat
// blocks (2 (2 nj)^2 + nj^2 doubles).  It grows with N: setup_hard refuses a horizon past the CU's LDS.
inline size_t hard_schur_lds_bytes(int N, int nj, int dmax) {
  return (size_t)N * (3 * nj * sizeof(double) + 2 * sizeof(int)) + (size_t)((dmax * 2 + 3) & ~3) * sizeof(int) +
         (size_t)(2 * 4 * nj * nj + nj * nj) * sizeof(double);
}
constexpr size_t CU_LDS_BYTES = 160 * 1024;   // gfx950: 160 KB of LDS per CU
int hard_set_max_lds();

// the dense PCG of tmpc_pcg_dense_batch (tmpc_pcg_dense.hip): PCG.pcg with any A / Pinv, D <= HARD_PCG_MAX_ROWS.
// A row-major [B][D][D] (the preconditioner builders read it), AT / PT column-major (A^T, Pinv^T: the PCG
// reads columns), Pd [B][D / nx][nx][nx] the builders' diagonal blocks
struct DenseArgs {
  int B, D, nx, precond, max_iter;
  double tol;
  const double *A, *b, *guess;
  double *AT, *PT, *Pd, *x, *trace_nu, *trace_res;
  int* iters;
  // past HARD_PCG_MAX_ROWS (launch_pcg_dense_big): the vectors in HBM scratch [B][D] and per-system state
  double *r, *p, *y, *q, *nu;
  int *done;
};
int launch_dense_transpose(hipStream_t s, int B, int D, const double* in, double* out);
int launch_dense_precond(hipStream_t s, const DenseArgs& a);
int launch_pcg_dense(hipStream_t s, const DenseArgs& a);
// the same PCG past HARD_PCG_MAX_ROWS rows: one launch per product / update phase, vectors in HBM, the same
// operation order (oracle/dense.py); host-synchronous every few iterations to stop once every system is done
int launch_pcg_dense_big(hipStream_t s, const DenseArgs& a);
int dense_set_max_lds();

}  // namespace tmpc
