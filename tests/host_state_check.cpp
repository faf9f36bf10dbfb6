// Stand-alone driver of csrc/tmpc_state.h, the solver state machine's scalar rules as the device kernels call
// them (tests/test_host_state.py compiles it with the host compiler's address / undefined-behaviour sanitizers
// and -ffp-contract=off, and compares its answers exactly with oracle/state.py).  One case per stdin line, one
// answer per stdout line, doubles as hex floats both ways:
//   opts  exit_tol alpha_factor alpha_min rho_factor rho_min rho_max rho_init exp_red_min exp_red_max mu max_iter
//   step  error deltaJ it rho drho     -> trace_rho rho drho exit_code done iter need_grad
//   sqp   merit Jn cn D al             -> mn ratio accept
//   ilqr  J Jn dV1 dV2 al              -> deltaJ ratio accept
//   outer max_c tol it max_iter changed -> exit_code iter exit_after_update
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "tmpc_state.h"

int main() {
  tmpc::SolverOpts o{};
  char line[512], kind[16];
  while (fgets(line, sizeof line, stdin)) {
    double v[10] = {0};
    int n = 0, used = 0, last = 0;
    if (sscanf(line, "%15s%n", kind, &used) != 1) continue;
    char* p = line + used;
    for (; n < 10; ++n) {   // the line's doubles; a trailing integer field follows for opts / outer
      char* end;
      const double d = strtod(p, &end);
      if (end == p) break;
      v[n] = d;
      p = end;
    }
    if (!strcmp(kind, "opts") && n == 10 && sscanf(p, "%d", &last) == 1) {
      o = tmpc::SolverOpts{v[0], v[1], v[2], v[3], v[4], v[5], v[6], v[7], v[8], v[9], last, 0};
      printf("opts\n");
    } else if (!strcmp(kind, "step") && n == 5) {
      const tmpc::StepOutcome r = tmpc::step_outcome(o, v[0] != 0.0, v[1], (int)v[2], v[3], v[4]);
      printf("step %a %a %a %d %d %d %d\n", r.trace_rho, r.rho, r.drho, r.exit_code, (int)r.done, r.iter, r.need_grad);
    } else if (!strcmp(kind, "sqp") && n == 5) {
      const tmpc::SqpTrial r = tmpc::sqp_trial(o, v[0], v[1], v[2], v[3], v[4]);
      printf("sqp %a %a %d\n", r.mn, r.ratio, (int)r.accept);
    } else if (!strcmp(kind, "ilqr") && n == 5) {
      const tmpc::IlqrTrial r = tmpc::ilqr_trial(o, v[0], v[1], v[2], v[3], v[4]);
      printf("ilqr %a %a %d\n", r.deltaJ, r.ratio, (int)r.accept);
    } else if (!strcmp(kind, "outer") && n == 5) {
      const tmpc::OuterExit r = tmpc::outer_exit(v[0], v[1], (int)v[2], (int)v[3]);
      printf("outer %d %d %d\n", r.exit_code, r.iter, tmpc::outer_exit_after_update(r.exit_code, v[4] != 0.0));
    } else {
      printf("bad line: %s", line);
      return 1;
    }
  }
  return 0;
}
