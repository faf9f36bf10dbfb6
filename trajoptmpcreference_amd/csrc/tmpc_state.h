// The per-problem solver state machine's scalar rules, written once: the line-search accept tests, the rho
// schedule (reduce_regularization, TrajoptMPCReference.py:457-461), the exit codes (check_for_exit_or_error,
// :463-481) and the soft-constraint outer loop's exit rule (:483-508).  tmpc_state.hip applies them to the device
// state; oracle/state.py states the same rules for the CPU oracle.
// Plain C++17, free of HIP headers: tests/host_state_check.cpp builds it with a plain C++ compiler.
#pragma once
#include <math.h>

#ifdef __HIPCC__
#define TMPC_HD __host__ __device__ inline
#else
#define TMPC_HD inline
#endif

namespace tmpc {

// set_default_options (TrajoptMPCReference.py:91-115) + the fixed merit weight mu = 10 (:545-546)
struct SolverOpts {
  double exit_tol_sqp, alpha_factor, alpha_min, rho_factor, rho_min, rho_max, rho_init, exp_red_min, exp_red_max, mu;
  int max_iter_sqp, pad;
};

// One SQP line-search trial (:655-666) at step length al: the trial's merit mn, the ratio of the merit's
// reduction to the expected one, and the accept test (an inf / NaN ratio compares false: rejected)
struct SqpTrial { double mn, ratio; bool accept; };
TMPC_HD SqpTrial sqp_trial(const SolverOpts& o, double merit, double Jn, double cn, double D, double al) {
  SqpTrial r;
  r.mn = Jn + o.mu * cn;
  const double dmerit = merit - r.mn;
  const double expected = al * (D - o.mu * cn);
  r.ratio = dmerit / expected;
  r.accept = dmerit >= 0.0 && r.ratio >= o.exp_red_min && r.ratio <= o.exp_red_max;
  return r;
}

// One iLQR trial (oracle/ilqr.py step): the cost's reduction over the backward sweep's expected one
struct IlqrTrial { double deltaJ, ratio; bool accept; };
TMPC_HD IlqrTrial ilqr_trial(const SolverOpts& o, double J, double Jn, double dV1, double dV2, double al) {
  IlqrTrial r;
  r.deltaJ = J - Jn;
  r.ratio = r.deltaJ / (-al * (dV1 + al * dV2));
  r.accept = r.ratio >= o.exp_red_min && r.ratio <= o.exp_red_max;
  return r;
}

// What iteration `it`'s line search (error: no trial accepted) makes of a problem: rho reduced on accept -- the
// value the trace row records -- and grown on error; exit 2 (rho past rho_max) / 1 (deltaJ below the tolerance) /
// 3 (the last iteration, which overrides them) / 0 (none: the problem goes on)
struct StepOutcome { double trace_rho, rho, drho; int exit_code, iter, need_grad; bool done; };
TMPC_HD StepOutcome step_outcome(const SolverOpts& o, bool error, double deltaJ, int it, double rho, double drho) {
  StepOutcome r;
  if (!error) {   // reduce_regularization
    drho = fmin(drho / o.rho_factor, 1.0 / o.rho_factor);
    rho = fmax(rho * drho, o.rho_min);
  }
  r.trace_rho = rho;
  r.exit_code = 0;
  if (error) {   // check_for_exit_or_error
    drho = fmax(drho * o.rho_factor, o.rho_factor);
    rho = fmax(rho * drho, o.rho_min);
    if (rho > o.rho_max) r.exit_code = 2;
  } else if (deltaJ < o.exit_tol_sqp) {
    r.exit_code = 1;
  }
  const bool last = it == o.max_iter_sqp - 1;
  if (last) r.exit_code = 3;
  r.rho = rho;
  r.drho = drho;
  r.done = r.exit_code != 0;
  r.iter = last ? it : it + 1;
  r.need_grad = (error || r.done) ? 0 : 1;
  return r;
}

// check_and_update_soft_constraints' exit rule for outer iteration `it`, before the constants' update: exit 1
// (max_c below the tolerance) / 2 (the last outer iteration, which overrides it) / 0, and the next outer_iter
struct OuterExit { int exit_code, iter; };
TMPC_HD OuterExit outer_exit(double max_c, double tol, int it, int max_iter) {
  const bool last = it == max_iter - 1;
  return {last ? 2 : max_c < tol ? 1 : 0, last ? it : it + 1};
}
// ... and after it: a pass that changed no constant (every mu at its limit) exits 3
TMPC_HD int outer_exit_after_update(int exit_code, bool changed) { return (exit_code == 0 && !changed) ? 3 : exit_code; }

}  // namespace tmpc
