// The solve loops' per-problem bookkeeping: the kernels that apply the state machine's scalar rules (tmpc_state.h) to
// the device state -- the decisions that end an SQP / iLQR iteration, the soft-constraint outer loop with a stream's
// slot hand-over, the resets a solve, a restarted pass or a refilled slot starts from -- and the batch's lists (alive
// list, counters, goal window).  None is a template over the model: the file compiles in seconds.  Per-problem
// control flow (line search, rho schedule, exit codes) is data, not host branches: every kernel takes the per-problem
// state and masks itself, the host only loops until no problem is active.
#include "tmpc_internal.h"

namespace tmpc {

// ======================================================================= workgroup copies
// One 64-lane workgroup moves a problem's rows (a trajectory is 768 doubles at arm6 N = 64) in the hand-over and the
// decisions' step application: written as `for (e = t; e < n; e += nt) dst[e] = src[e]`, each pass's load waited for
// the previous pass's store whenever the compiler could not prove the two rows apart (struct members carry no
// __restrict__), so a row cost n / nt dependent memory round trips -- the slowest workgroup of these launches set
// their ~30-70 us (profiles/r06/counters).  Here U passes' loads are issued before any of their stores: one round
// trip per U passes.  Every element is the same expression of the same operands: the values are unchanged bit for bit.
// for e in [0, n) step nt from t: st(e, ld(e)), U elements per lane loaded before any is stored
template <int U, class V, class LD, class ST>
__device__ __forceinline__ void wg_batched(int n, int t, int nt, LD ld, ST st) {
  for (int b0 = t; b0 < n; b0 += U * nt) {
    V v[U];
#pragma unroll
    for (int j = 0; j < U; ++j) {
      const int e = b0 + j * nt;
      v[j] = e < n ? ld(e) : V(0);
    }
#pragma unroll
    for (int j = 0; j < U; ++j) {
      const int e = b0 + j * nt;
      if (e < n) st(e, v[j]);
    }
  }
}

// dst[e] = src[e], e in [0, n)
template <int U, class V>
__device__ __forceinline__ void wg_copy(V* dst, const V* src, int n, int t, int nt) {
  wg_batched<U, V>(n, t, nt, [&](int e) { return src[e]; }, [&](int e, V v) { dst[e] = v; });
}

// ======================================================================= the resets and trace rows, once
// The state an inner loop starts from (a fresh solve, a restarted pass, a refilled slot); the caller sets
// st.active, which differs between the three.
__device__ __forceinline__ void reset_state(const ProbState& st, int b, double rho_init) {
  st.rho[b] = rho_init;
  st.drho[b] = 1.0;
  st.iter[b] = 0;
  st.need_grad[b] = 1;
  st.exit_sqp[b] = 0;
}

__device__ __forceinline__ void reset_outer(int b, int* outer_active, int* outer_iter, int* exit_soft) {
  outer_active[b] = 1; outer_iter[b] = 0; exit_soft[b] = 0;
}

// (soft_initial, the constants a soft slot starts from: tmpc_internal.h, shared with the MPC step's advance kernel)

// the trace row of an iteration (:691-705 / :729-743)
__device__ __forceinline__ void trace_step_row(const TraceDev& tr, size_t e, int it, int ls, double al, double rho,
                                               double J, double c, double merit, double D, double ratio,
                                               bool accepted, int pcg_iters, int singular) {
  tr.iteration[e] = it; tr.ls_iter[e] = ls; tr.alpha[e] = al; tr.rho[e] = rho;
  tr.J[e] = J; tr.c[e] = c; tr.merit[e] = merit;
  tr.D[e] = D; tr.ratio[e] = ratio; tr.accepted[e] = accepted ? 1 : 0;
  tr.pcg_iters[e] = pcg_iters; tr.singular[e] = singular;
}

// trace row 0 of a pass: the initial merit / cost (:555-569)
__device__ __forceinline__ void trace_row0(const TraceDev& tr, size_t e, double rho, double J, double c, double merit) {
  trace_step_row(tr, e, 0, 0, 1.0, rho, J, c, merit, __builtin_nan(""), __builtin_nan(""), false, 0, 0);
}

// an iteration's outcome (tmpc_state.h) into the problem's state and the count of live problems
__device__ __forceinline__ void store_outcome(const ProbState& st, int b, const StepOutcome& r,
                                              int* __restrict__ active_count) {
  if (r.exit_code) st.exit_sqp[b] = r.exit_code;
  st.iter[b] = r.iter; st.rho[b] = r.rho; st.drho[b] = r.drho; st.need_grad[b] = r.need_grad;
  if (r.done) st.active[b] = 0;
  else *active_count = 1;   // the host only tests for zero
}

// ======================================================================= line-search decision + state machine
// One workgroup per problem.  Reproduces the accept test (:655-666), the alpha schedule (:712-718),
// reduce_regularization (:457-461) and check_for_exit_or_error (:463-481), applies the accepted step and records
// the trace row (:691-705 / :729-743).
__global__ void __launch_bounds__(64) k_ls_decide(PList P, int B, int N, int NX, int NU, int T, int mode, int soft,
                                                  const double* __restrict__ alphas, SolverOpts o,
                                                  const double* __restrict__ terms, double* __restrict__ x,
                                                  double* __restrict__ u, const double* __restrict__ dx,
                                                  const double* __restrict__ du, ProbState st,
                                                  const int* __restrict__ pcg_iters, TraceDev tr,
                                                  int* __restrict__ active_count,
                                                  unsigned long long* __restrict__ counters,
                                                  const double* __restrict__ hterms,
                                                  const int* __restrict__ qp_singular,
                                                  int* __restrict__ activate, int stage_bytes) {
  if (!P.has(blockIdx.x, B)) return;
  const int b = P.at(blockIdx.x);
  if (!st.active[b]) return;
  __shared__ double sJ[64], sC[64], sD[64], s_al[64];
  __shared__ int s_choice;
  const int t = threadIdx.x;
  if (t < T) s_al[t] = alphas[t];   // (published by the barrier after the sums)
  // the problem's line-search terms staged in LDS by all 64 lanes at once (dynamic LDS of T N 4 + T N
  // doubles when the launch gives it, LS_DECIDE_STAGE_MAX): one round of independent loads instead of the
  // trial lanes' serial walks through HBM; the sums below read the same values in the same order
  extern __shared__ double s_terms[];
  const bool staged = stage_bytes > 0;
  if (staged) {
    const double* src = terms + (size_t)b * T * N * 4;
    const int ne = T * N * 4;
    // 18 passes' loads in flight (36 per lane at T = 9, N = 64: two round trips; 8 took five)
#pragma unroll 18
    for (int e = t; e < ne; e += 64) s_terms[e] = src[e];
    if (hterms) {
      const double* hs = hterms + (size_t)b * T * N;
#pragma unroll 4
      for (int e = t; e < T * N; e += 64) s_terms[ne + e] = hs[e];
    }
    __syncthreads();
  }
  if (t < T) {
    const double* tm = staged ? s_terms + (size_t)t * N * 4 : terms + ((size_t)b * T + t) * N * 4;
    double J = 0.0, c = 0.0, D = 0.0;
    for (int k = 0; k < N - 1; ++k) J = J + tm[k * 4 + 0];
    J = J + tm[(N - 1) * 4 + 0];
    if (soft) {   // totalCost adds the soft values after the cost terms (:303-307)
      for (int k = 0; k < N - 1; ++k) J = J + tm[k * 4 + 3];
      J = J + tm[(N - 1) * 4 + 3];
    }
    c = tm[(N - 1) * 4 + 1];
    for (int k = 0; k < N - 1; ++k) c = c + tm[k * 4 + 1];
    for (int k = 0; k < N - 1; ++k) D += tm[k * 4 + 2];
    D += tm[(N - 1) * 4 + 2];
    if (hterms) {   // hard box-constraint terms after the dynamics ones, knot by knot (:286-293)
      const double* th = staged ? s_terms + (size_t)T * N * 4 + (size_t)t * N : hterms + ((size_t)b * T + t) * N;
      for (int k = 0; k < N; ++k) c = c + th[k];
    }
    sJ[t] = J; sC[t] = c; sD[t] = D;
  }
  __syncthreads();
  const int W = o.max_iter_sqp + 1;
  if (t == 0) {
    if (mode == LS_MODE_INIT) {
      const double J = sJ[0], c = sC[0];
      const double merit = J + o.mu * c;
      st.J[b] = J; st.c[b] = c; st.merit[b] = merit;
      trace_row0(tr, (size_t)b * W, st.rho[b], J, c, merit);
      if (activate) {   // a restarted pass / a stream's new problem enters its inner loop (st.active: act_init)
        st.active[b] = 0;
        activate[b] = 1;
      }
      s_choice = -2;
    } else {
      const double J = st.J[b], c = st.c[b], merit = st.merit[b];
      const double rho = st.rho[b], drho = st.drho[b];   // (read ahead of the stores below, which may alias them)
      int choice = -1, ls = 0;
      // a failed search keeps the last trial's values
      double D = 0.0, Jn = 0.0, cn = 0.0, al = 1.0;
      SqpTrial q{0.0, 0.0, false};
      for (int tt = 0; tt < T; ++tt) {
        al = s_al[tt]; ls = tt; Jn = sJ[tt]; cn = sC[tt]; D = sD[tt];
        q = sqp_trial(o, merit, Jn, cn, D, al);
        if (q.accept) { choice = tt; break; }
      }
      const int it = st.iter[b];
      if (counters) {
        // per-problem tallies [B][3], summed once per solve by k_sum_counters (one global
        // atomic per problem and iteration serialised thousands of blocks on one L2 line):
        // [0] problem-QPs solved, [1] PCG iterations, [2] QPs with a fresh dynamics gradient
        unsigned long long* pc = counters + (size_t)b * 3;
        pc[0] += 1ull;
        pc[1] += (unsigned long long)(pcg_iters ? pcg_iters[b] : 0);
        pc[2] += (unsigned long long)st.need_grad[b];
      }
      const bool error = choice < 0;
      if (!error) { st.J[b] = Jn; st.c[b] = cn; st.merit[b] = q.mn; }
      const StepOutcome r = step_outcome(o, error, J - Jn, it, rho, drho);   // (J - Jn: read on accept only)
      trace_step_row(tr, (size_t)b * W + it + 1, it, ls, al, r.trace_rho, error ? J : Jn, error ? c : cn,
                     error ? merit : q.mn, D, q.ratio, !error, pcg_iters ? pcg_iters[b] : 0,
                     qp_singular ? qp_singular[b] : 0);
      store_outcome(st, b, r, active_count);
      s_choice = choice;
    }
  }
  __syncthreads();
  const int choice = s_choice;
  if (choice >= 0) {
    const double al = alphas[choice];
    double* xb = x + (size_t)b * NX * N;
    const double* dxb = dx + (size_t)b * N * NX;
    // x - alpha dx, u - alpha du element by element, the loads of U passes ahead of their stores (wg_batched)
    wg_batched<12, double>(NX * N, t, blockDim.x, [&](int e) {
      const int m = e / N, k = e - m * N;
      return xb[e] - al * dxb[k * NX + m];
    }, [&](int e, double v) { xb[e] = v; });
    const int K = N - 1;
    double* ub = u + (size_t)b * NU * K;
    const double* dub = du + (size_t)b * K * NU;
    wg_batched<8, double>(NU * K, t, blockDim.x, [&](int e) {
      const int m = e / K, k = e - m * K;
      return ub[e] - al * dub[k * NU + m];
    }, [&](int e, double v) { ub[e] = v; });
  } else if (choice == -2 && t == 0) {
    *active_count = 1;
  }
}

void launch_ls_decide(hipStream_t s, const DecideArgs& a) {
  // LDS staging of the terms up to LS_DECIDE_STAGE_MAX bytes (within the default dynamic-LDS limit; N = 64,
  // T = 9: 18 kB), the direct HBM walks past it
  constexpr size_t LS_DECIDE_STAGE_MAX = 60 * 1024;
  size_t stage = ((size_t)a.T * a.N * 4 + (a.hterms ? (size_t)a.T * a.N : 0)) * sizeof(double);
  if (stage > LS_DECIDE_STAGE_MAX) stage = 0;
  hipLaunchKernelGGL(k_ls_decide, dim3(a.B), dim3(64), stage, s, a.P, a.B, a.N, a.NX, a.NU, a.T, a.mode, a.soft, a.alphas,
                     a.o, a.terms, a.x, a.u, a.dx, a.du, a.st, a.pcg_iters, a.tr, a.active_count, a.counters, a.hterms,
                     a.qp_singular, a.activate, (int)stage);
}

// ======================================================================= iLQR decision + state machine
// One 64-lane workgroup per problem.  Acceptance ratio (J - J^) / (-alpha (dV1 + alpha dV2)) in
// [exp_red_min, exp_red_max] in the reference's alpha order (oracle/ilqr.py), rho schedule and exit
// codes of reduce_regularization / check_for_exit_or_error (:457-481), trace row, trajectory copy.
__global__ void __launch_bounds__(64) k_ilqr_decide(PList P, int B, int N, int NX, int NU, int T, int init,
                                                    const double* __restrict__ alphas, SolverOpts o,
                                                    const double* __restrict__ Jt, const double* __restrict__ dV,
                                                    const int* __restrict__ okb, const double* __restrict__ xt,
                                                    const double* __restrict__ ut, double* __restrict__ x,
                                                    double* __restrict__ u, ProbState st, TraceDev tr,
                                                    int* __restrict__ active_count,
                                                    unsigned long long* __restrict__ counters,
                                                    int* __restrict__ activate) {
  if (!P.has(blockIdx.x, B)) return;
  const int b = P.at(blockIdx.x);
  if (!st.active[b]) return;
  __shared__ int s_choice;
  __shared__ double s_al[64], s_J[64];
  const int t = threadIdx.x;
  const int W = o.max_iter_sqp + 1;
  const int K = N - 1;
  if (t < T) {   // the trials' alphas and costs loaded by their lanes at once (lane 0 walks them below)
    s_al[t] = alphas[t];
    s_J[t] = Jt[(size_t)b * T + t];
  }
  __syncthreads();
  if (t == 0) {
    if (init) {
      const double J = s_J[0];
      st.J[b] = J; st.c[b] = 0.0; st.merit[b] = J;
      trace_row0(tr, (size_t)b * W, st.rho[b], J, 0.0, J);
      *active_count = 1;   // the host only tests for zero
      if (activate) {      // a restarted pass / a stream's new problem enters its inner loop (st.active: act_init)
        st.active[b] = 0;
        activate[b] = 1;
      }
      s_choice = -1;
    } else {
      const double J = st.J[b], rho = st.rho[b], drho = st.drho[b];
      const bool bok = okb[b] != 0;
      const double dV1 = dV[2 * b], dV2 = dV[2 * b + 1];
      int choice = -1, ls = 0;   // a failed search keeps the last trial's values; a failed sweep (!bok) has no trial
      double al = 0.0, Jn = J;
      IlqrTrial q{0.0, __builtin_nan(""), false};
      if (bok) {
        for (int tt = 0; tt < T; ++tt) {
          al = s_al[tt]; ls = tt; Jn = s_J[tt];
          q = ilqr_trial(o, J, Jn, dV1, dV2, al);
          if (q.accept) { choice = tt; break; }
        }
      }
      const bool error = choice < 0;
      const int it = st.iter[b];
      if (counters) {
        // per-problem tallies [B][3], summed once per solve (k_sum_counters): [0] problem-iterations,
        // [2] iterations with a fresh dynamics gradient (same-address atomics serialised the launch)
        unsigned long long* pc = counters + (size_t)b * 3;
        pc[0] += 1ull;
        pc[2] += (unsigned long long)st.need_grad[b];
      }
      if (!error) st.J[b] = st.merit[b] = Jn;
      const StepOutcome r = step_outcome(o, error, q.deltaJ, it, rho, drho);
      // (singular: 0, the value alloc_trace leaves in a column iLQR never sets)
      trace_step_row(tr, (size_t)b * W + it + 1, it, bok ? ls : 0, bok ? al : 0.0, r.trace_rho, error ? J : Jn, 0.0,
                     error ? J : Jn, bok ? dV1 : __builtin_nan(""), bok ? q.ratio : __builtin_nan(""), !error, 0, 0);
      store_outcome(st, b, r, active_count);
      s_choice = choice;
    }
  }
  __syncthreads();
  const int choice = s_choice;
  if (choice >= 0) {
    const double* xs_ = xt + ((size_t)b * T + choice) * NX * N;
    const double* us_ = ut + ((size_t)b * T + choice) * NU * K;
    // trial trajectories are knot-major ([k][m], see k_ilqr_forward); x / u the reference's [m][k]; the
    // loads of U passes ahead of their stores (wg_batched)
    double* xb = x + (size_t)b * NX * N;
    double* ub = u + (size_t)b * NU * K;
    wg_batched<12, double>(NX * N, t, 64, [&](int e) {
      const int m = e / N, k = e - m * N;
      return xs_[k * NX + m];
    }, [&](int e, double v) { xb[e] = v; });
    wg_batched<8, double>(NU * K, t, 64, [&](int e) {
      const int m = e / K, k = e - m * K;
      return us_[k * NU + m];
    }, [&](int e, double v) { ub[e] = v; });
  }
}

void launch_ilqr_decide(hipStream_t s, const DecideArgs& a) {
  hipLaunchKernelGGL(k_ilqr_decide, dim3(a.B), dim3(64), 0, s, a.P, a.B, a.N, a.NX, a.NU, a.T, a.init, a.alphas, a.o, a.Jt,
                     a.dV, a.ok, a.xt, a.ut, a.x, a.u, a.st, a.tr, a.active_count, a.counters, a.activate);
}

// Sum the per-problem tallies of k_ls_decide into out[0..2] (256 atomics per solve).
__global__ void __launch_bounds__(256) k_sum_counters(int B, const unsigned long long* __restrict__ pc,
                                                      unsigned long long* __restrict__ out) {
  unsigned long long s0 = 0, s1 = 0, s2 = 0;
  for (int b = threadIdx.x; b < B; b += blockDim.x) {
    s0 += pc[(size_t)b * 3];
    s1 += pc[(size_t)b * 3 + 1];
    s2 += pc[(size_t)b * 3 + 2];
  }
  atomicAdd(&out[0], s0);
  atomicAdd(&out[1], s1);
  atomicAdd(&out[2], s2);
}

void launch_sum_counters(hipStream_t s, int B, const unsigned long long* pc, unsigned long long* out) {
  hipLaunchKernelGGL(k_sum_counters, dim3(1), dim3(256), 0, s, B, pc, out);
}

__global__ void k_init_state(int B, double rho_init, ProbState st, const int* __restrict__ outer_active) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  if (outer_active && !outer_active[b]) {
    st.active[b] = 0;
    return;
  }
  reset_state(st, b, rho_init);
  st.active[b] = 1;
}

void launch_init_state(hipStream_t s, int B, double rho_init, const ProbState& st, const int* outer_active) {
  hipLaunchKernelGGL(k_init_state, TMPC_GRID(B, 256), 0, s, B, rho_init, st, outer_active);
}

// The problems still alive in the lock-step loop (mask != 0), ascending, and their count: one
// 1024-lane workgroup, each lane a contiguous chunk of the batch, a block prefix sum of the chunk
// counts.  host_slot (nullable): the count also lands in the iteration's flag slot the host reads back.
__global__ void __launch_bounds__(1024) k_alive_list(int B, const int* __restrict__ alive, int* __restrict__ idx,
                                                     int* __restrict__ cnt, int* __restrict__ host_slot) {
  __shared__ int part[1024];
  const int t = threadIdx.x, nt = blockDim.x;
  const int chunk = (B + nt - 1) / nt;
  const int lo = t * chunk, hi = min(B, lo + chunk);
  int c = 0;
  for (int b = lo; b < hi; ++b) c += alive[b] != 0;
  part[t] = c;
  __syncthreads();
  for (int off = 1; off < nt; off <<= 1) {   // inclusive Hillis-Steele scan
    const int v = t >= off ? part[t - off] : 0;
    __syncthreads();
    part[t] += v;
    __syncthreads();
  }
  int o = part[t] - c;
  for (int b = lo; b < hi; ++b)
    if (alive[b]) idx[o++] = b;
  if (t == nt - 1) {
    // the lock-step loop sizes its grids by an earlier length (tmpc_api.cpp lockstep_loop): valid only
    // while the list never grows -- host_slot[1] flags a violation, which the host turns into an error
    if (host_slot) {
      host_slot[0] = part[t];
      if (part[t] > *cnt) host_slot[1] = 1;
    }
    *cnt = part[t];
  }
}

void launch_alive_list(hipStream_t s, int B, const int* alive, int* idx, int* cnt, int* host_slot) {
  hipLaunchKernelGGL(k_alive_list, dim3(1), dim3(1024), 0, s, B, alive, idx, cnt, host_slot);
}

// ======================================================================= soft-constraint outer loop
// check_and_update_soft_constraints (TrajoptMPCReference.py:483-508) for one problem per 64-lane workgroup, after its
// inner SQP loop exited:
//   max_c = max over types and knots of |min(v)|  (max_soft_constraint_value, :130-135)
//   the exit rule of tmpc_state.h (outer_exit); when it goes on, update_soft_constraint_constants (:137-166)
//   elementwise, and exit 3 when no constant changed (all mu at their limit).
// Unconstrained problems (no soft type) take the reference's path: max_c = 0 -> exit 1.
// Two drivers:
//   lock-step (inner == null): every problem still in the outer loop, after the whole batch's inner loops have
//     exited; *outer_count = 1 when some problem continues;
//   per-problem (inner = the inner loop's active flags): only problems whose inner loop has just exited (outer_active
//     && !inner && !init); one that continues is reset for its next pass (reset_state) and flagged in act_init for its
//     initial merit evaluation, so each problem runs its passes back to back instead of waiting for the slowest pass.
__device__ __forceinline__ double soft_v(const ConstrDev* Cs, int t, int e, int n, double z) {
  const int i = e < n ? e : e - n;
  return e < n ? z - Cs->lb[t][i] : Cs->ub[t][i] - z;
}

// A stream's hand-over of slot s, whose problem has just left its outer loop (tmpc_internal.h StreamDev),
// by the workgroup of k_soft_outer that ended it: the finished problem's trajectory, status and trace rows
// to its output rows; then, when a problem is pending, its x, u, x[:, 0] and the state a fresh solve
// starts from -- reset_state, reset_outer, the soft constants' initial values, a zero PCG warm start -- and
// act_init, so that its initial merit / cost is evaluated this iteration.
__device__ void stream_handover(int s, const StreamDev& sd, double* __restrict__ x, double* __restrict__ u,
                                double* __restrict__ xs, const ProbState& st, int* __restrict__ outer_active,
                                int* __restrict__ outer_iter, int* __restrict__ exit_soft,
                                int* __restrict__ act_init, double rho_init, const TraceDev& tr,
                                const ConstrDev* __restrict__ Cs, double* __restrict__ mu, double* __restrict__ lam,
                                double* __restrict__ phi, double* __restrict__ lam_warm) {
  __shared__ int s_next;
  const int t = threadIdx.x, nt = blockDim.x;
  const int old_l = sd.slot_pid[s];
  const int old = sd.pbase + old_l;   // the output row (global problem index)
  const int XN = sd.NX * sd.N, UN = sd.NU * (sd.N - 1), W = sd.W;
  double* xb = x + (size_t)s * XN;
  double* ub = u + (size_t)s * UN;
  if (t == 0) s_next = atomicAdd(sd.next, 1);
  if (old_l >= 0) {
    // the rows' loads batched ahead of their stores (wg_batched): 12 + 6 passes at arm6 N = 64 were
    // that many dependent round trips
    if (sd.x_out) wg_copy<12>(sd.x_out + (size_t)old * XN, xb, XN, t, nt);
    if (sd.u_out) wg_copy<8>(sd.u_out + (size_t)old * UN, ub, UN, t, nt);
    if (sd.status && t == 0) {
      int* so = sd.status + (size_t)old * 4;
      so[0] = st.exit_sqp[s];
      so[1] = st.iter[s];
      so[2] = exit_soft[s];
      so[3] = outer_iter[s];
    }
    const TraceDev& to = sd.tr_out;
    const size_t ri = (size_t)s * W, ro = (size_t)old * W;
#define TMPC_TR_COPY(f) \
  if (to.f) wg_copy<4>(to.f + ro, tr.f + ri, W, t, nt);
    TMPC_TR_COPY(iteration) TMPC_TR_COPY(ls_iter) TMPC_TR_COPY(alpha) TMPC_TR_COPY(rho) TMPC_TR_COPY(J)
    TMPC_TR_COPY(c) TMPC_TR_COPY(merit) TMPC_TR_COPY(D) TMPC_TR_COPY(ratio) TMPC_TR_COPY(accepted)
    TMPC_TR_COPY(pcg_iters) TMPC_TR_COPY(singular)
#undef TMPC_TR_COPY
  }
  __syncthreads();   // every read of the finished problem precedes the writes of the next one
  const int nw = s_next;
  if (nw >= sd.P) {
    if (t == 0) sd.slot_pid[s] = -1;
    return;
  }
  const size_t src = (size_t)((sd.pbase + nw) % sd.period);
  wg_copy<12>(xb, sd.x_in + src * XN, XN, t, nt);
  wg_copy<8>(ub, sd.u_in + src * UN, UN, t, nt);
  for (int m = t; m < sd.NX; m += nt) xs[(size_t)s * sd.NX + m] = sd.x_in[src * XN + (size_t)m * sd.N];
  if (mu) {
    const int MC = sd.MC;
    for (int i = t; i < sd.N * MC; i += nt) {
      const SoftInit si = soft_initial(Cs, (i % MC) / (MC / 3));
      const size_t o = (size_t)s * sd.N * MC + i;
      mu[o] = si.mu; lam[o] = si.lam; phi[o] = si.phi;
    }
  }
  if (lam_warm)
    for (int e = t; e < sd.NX * sd.N; e += nt) lam_warm[(size_t)s * sd.NX * sd.N + e] = 0.0;
  if (t == 0) {
    reset_state(st, s, rho_init);
    st.active[s] = 0;   // set by the initial merit's decision (act_init)
    reset_outer(s, outer_active, outer_iter, exit_soft);
    act_init[s] = 1;
    sd.slot_pid[s] = nw;
  }
}

__global__ void __launch_bounds__(64) k_soft_outer(const ConstrDev* __restrict__ Cs, PList P, int B, int N, int NJ,
                                                   double tol, int max_iter, double* __restrict__ x,
                                                   double* __restrict__ u, double* __restrict__ mu,
                                                   double* __restrict__ lam, double* __restrict__ phi,
                                                   int* __restrict__ outer_active, int* __restrict__ outer_iter,
                                                   int* __restrict__ exit_soft, int* __restrict__ outer_count,
                                                   ProbState st, int* __restrict__ act_init, double rho_init,
                                                   StreamDev sd, double* __restrict__ xs, TraceDev tr,
                                                   double* __restrict__ lam_warm) {
  if (!P.has(blockIdx.x, B)) return;
  const int b = P.at(blockIdx.x);
  if (!outer_active[b]) return;
  const bool per_problem = act_init != nullptr;
  if (per_problem && (st.active[b] || act_init[b])) return;
  const int t0 = threadIdx.x;
  const int NX = 2 * NJ, K = N - 1, MC = 6 * NJ;
  const double* xb = x + (size_t)b * NX * N;
  const double* ub = u + (size_t)b * NJ * K;
  auto zval = [&](int t, int i, int k) -> double {
    return t == 2 ? ub[i * K + k] : xb[(t * NJ + i) * N + k];
  };
  // max_c over (type, knot) pairs (the pair's 2 n values loaded together, then reduced in order); PB pairs'
  // loads per lane issued before any is reduced (one round trip for arm6 N = 64's three passes)
  double mx = 0.0;
  constexpr int PB = 4;
  for (int p0 = t0; p0 < 3 * N; p0 += 64 * PB) {
    double zz[PB][NJMAX];
    bool okp[PB];
#pragma unroll
    for (int j = 0; j < PB; ++j) {
      const int p = p0 + 64 * j;
      const int t = p / N, k = p - t * N;
      okp[j] = p < 3 * N && Cs->mode[t] != SOFT_NONE && !(t == 2 && k == K);
#pragma unroll
      for (int i = 0; i < NJMAX; ++i) zz[j][i] = (okp[j] && i < NJ) ? zval(t, i, k) : 0.0;
    }
#pragma unroll
    for (int j = 0; j < PB; ++j) {
      if (!okp[j]) continue;
      const int t = (p0 + 64 * j) / N;
      // the lower bounds' values, then the upper ones' (e = i, then NJ + i): the pair's order, with
      // static indices into zz (NJ is a launch argument: zz[e - NJ] had put zz in scratch)
      double mn = 0.0;
#pragma unroll
      for (int i = 0; i < NJMAX; ++i) {
        if (i >= NJ) break;
        const double v = soft_v(Cs, t, i, NJ, zz[j][i]);
        mn = i == 0 ? v : fmin(mn, v);
      }
#pragma unroll
      for (int i = 0; i < NJMAX; ++i) {
        if (i >= NJ) break;
        mn = fmin(mn, soft_v(Cs, t, NJ + i, NJ, zz[j][i]));
      }
      mx = fmax(mx, fabs(mn));
    }
  }
  __shared__ double smax[64];
  __shared__ int s_exit, s_changed, s_done;
  smax[t0] = mx;
  if (t0 == 0) s_changed = 0;
  __syncthreads();
  if (t0 == 0) {
    double m = 0.0;
    for (int i = 0; i < 64; ++i) m = fmax(m, smax[i]);
    const OuterExit r = outer_exit(m, tol, outer_iter[b], max_iter);
    outer_iter[b] = r.iter;
    s_exit = r.exit_code;
  }
  __syncthreads();
  if (s_exit == 0) {
    // update_soft_constraint_constants entry by entry; OB entries per lane have their loads issued together
    // before any of them is updated (each entry's arithmetic is unchanged)
    constexpr int OB = 18;
    for (int p0 = t0; p0 < N * MC; p0 += 64 * OB) {
      double zv[OB], ph[OB], mv[OB], lv[OB];
      bool ok[OB];
#pragma unroll
      for (int j = 0; j < OB; ++j) {
        const int p = p0 + 64 * j;
        const int k = p / MC, sl = p - k * MC;
        const int t = sl / (2 * NJ), e = sl - t * 2 * NJ;
        ok[j] = p < N * MC && Cs->mode[t] != SOFT_NONE && !(t == 2 && k == K);
        zv[j] = ph[j] = mv[j] = lv[j] = 0.0;
        if (ok[j]) {
          const size_t o = ((size_t)b * N + k) * MC + sl;
          zv[j] = zval(t, e < NJ ? e : e - NJ, k);
          ph[j] = phi[o];
          mv[j] = mu[o];
          lv[j] = lam[o];
        }
      }
#pragma unroll
      for (int j = 0; j < OB; ++j) {
        if (!ok[j]) continue;
        const int p = p0 + 64 * j;
        const int k = p / MC, sl = p - k * MC;
        const int t = sl / (2 * NJ), e = sl - t * 2 * NJ;
        const double v = soft_v(Cs, t, e, NJ, zv[j]);
        const size_t o = ((size_t)b * N + k) * MC + sl;
        if (v < 0.0 && !(fabs(v) < ph[j])) {
          if (mv[j] < Cs->mu_max[t]) {
            s_changed = 1;
            mu[o] = fmin(Cs->mu_max[t], mv[j] * Cs->mu_factor[t]);
          }
        } else if (v < 0.0) {
          s_changed = 1;
          lam[o] = lv[j] + mv[j] * v;
          phi[o] = ph[j] / Cs->phi_factor[t];
        }
      }
    }
  }
  __syncthreads();
  if (t0 == 0) {
    const int ex = outer_exit_after_update(s_exit, s_changed != 0);
    s_done = ex != 0;
    if (ex) {
      exit_soft[b] = ex;
      outer_active[b] = 0;
    } else {
      *outer_count = 1;   // the host only tests for zero
      if (per_problem) {  // next pass (st.active stays 0 until the initial merit's decision: act_init)
        reset_state(st, b, rho_init);
        act_init[b] = 1;
      }
    }
  }
  if (sd.P > 0) {   // a stream (per-problem mode): a finished problem hands its slot on
    __syncthreads();
    if (s_done)
      stream_handover(b, sd, x, u, xs, st, outer_active, outer_iter, exit_soft, act_init, rho_init, tr, Cs, mu, lam,
                      phi, lam_warm);
  }
}

void launch_soft_outer(hipStream_t s, const SoftOuterArgs& a) {
  hipLaunchKernelGGL(k_soft_outer, dim3(a.B), dim3(64), 0, s, a.Cs, a.P, a.B, a.N, a.nj, a.tol, a.max_iter, a.x, a.u, a.mu,
                     a.lam, a.phi, a.outer_active, a.outer_iter, a.exit_soft, a.outer_count, a.st, a.act_init, a.rho_init,
                     a.sd, a.xs, a.tr, a.lam_warm);
}

__global__ void k_soft_init(const ConstrDev* __restrict__ Cs, size_t total, int MC, double* __restrict__ mu,
                            double* __restrict__ lam, double* __restrict__ phi) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) return;
  const SoftInit si = soft_initial(Cs, (int)(i % MC) / (MC / 3));
  mu[i] = si.mu; lam[i] = si.lam; phi[i] = si.phi;
}

void launch_soft_init(hipStream_t s, const ConstrDev* Cs, size_t total, int MC, double* mu, double* lam,
                      double* phi) {
  hipLaunchKernelGGL(k_soft_init, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, Cs, total, MC, mu, lam,
                     phi);
}

__global__ void k_outer_init(int B, int* __restrict__ outer_active, int* __restrict__ outer_iter,
                             int* __restrict__ exit_soft) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  reset_outer(b, outer_active, outer_iter, exit_soft);
}

void launch_outer_init(hipStream_t s, int B, int* outer_active, int* outer_iter, int* exit_soft) {
  hipLaunchKernelGGL(k_outer_init, TMPC_GRID(B, 256), 0, s, B, outer_active, outer_iter, exit_soft);
}

// ======================================================================= continuous batching (tmpc_internal.h)
// slot s starts with problem s: one 256-thread workgroup per slot copies its inputs (x, u are read and
// written with unit stride, so a workgroup's loads and stores coalesce)
__global__ void __launch_bounds__(256) k_stream_init(int B, StreamDev sd, double* __restrict__ x,
                                                     double* __restrict__ u) {
  const int s = blockIdx.x, t = threadIdx.x;
  const int XN = sd.NX * sd.N, UN = sd.NU * (sd.N - 1);
  const size_t src = (size_t)((sd.pbase + s) % sd.period);
  wg_copy<4>(x + (size_t)s * XN, sd.x_in + src * XN, XN, t, blockDim.x);
  wg_copy<4>(u + (size_t)s * UN, sd.u_in + src * UN, UN, t, blockDim.x);
  if (t == 0) {
    sd.slot_pid[s] = s;
    if (s == 0) *sd.next = B;   // the next pending problem (stream_handover takes them with atomics)
  }
}

void launch_stream_init(hipStream_t s, int B, const StreamDev& sd, double* x, double* u) {
  hipLaunchKernelGGL(k_stream_init, dim3(B), dim3(256), 0, s, B, sd, x, u);
}

// ======================================================================= goal window (tmpc_internal.h)
// One workgroup per problem resolves the reference xref [R][nx][M] (the layout of x) into the problem's rows of
// the knot-major window gw [B][N][nx]: row (pbase + problem) % R, column min(k + step, M - 1).  Run once per
// horizon solve (and for a stream's refilled slots), so the goal-reading kernels take one pointer and know
// nothing of R, M or the step.  The stores are unit-stride; the reads stride by M, once.
__global__ void __launch_bounds__(256) k_goal_window(int B, int N, int nx, int R, int M, int step,
                                                     const double* __restrict__ xref, const int* __restrict__ pid,
                                                     int pbase, const int* __restrict__ mask,
                                                     double* __restrict__ gw) {
  const int b = blockIdx.x;
  if (b >= B || (mask && !mask[b])) return;
  const int p = pid ? pid[b] : b;
  if (p < 0) return;
  const double* row = xref + (size_t)((pbase + p) % R) * nx * M;
  double* out = gw + (size_t)b * N * nx;
  for (int e = threadIdx.x; e < N * nx; e += blockDim.x) {
    const int k = e / nx, m = e - k * nx;
    const long long c = (long long)k + step;
    out[e] = row[(size_t)m * M + (size_t)(c < M - 1 ? c : M - 1)];
  }
}

void launch_goal_window(hipStream_t s, const GoalWindowArgs& a) {
  hipLaunchKernelGGL(k_goal_window, dim3(a.B), dim3(256), 0, s, a.B, a.N, a.nx, a.R, a.M, a.step, a.xref, a.pid, a.pbase,
                     a.mask, a.gw);
}

}  // namespace tmpc
