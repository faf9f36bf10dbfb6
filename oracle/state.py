"""The solver state machine's scalar rules, once for sqp() and ilqr(): the line-search accept tests, what an
iteration's line search makes of rho and the exit code (reduce_regularization and check_for_exit_or_error,
TrajoptMPCReference.py:457-481), and the soft-constraint outer loop's exit rule (:483-508).  The device states
the same rules in csrc/tmpc_state.h; tests/test_host_state.py compares the two exactly."""
import numpy as np


def _ratio(num, den):
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.float64(num) / np.float64(den)


def sqp_trial(o, merit, J_new, c_new, D, alpha, mu):
    """One SQP line-search trial (:655-666): (merit_new, ratio, accepted)."""
    merit_new = J_new + mu * c_new
    delta_merit = merit - merit_new
    ratio = _ratio(delta_merit, alpha * (D - mu * c_new))
    return merit_new, ratio, bool(delta_merit >= 0 and ratio >= o["expected_reduction_min_SQP_DDP"]
                                  and ratio <= o["expected_reduction_max_SQP_DDP"])


def ilqr_trial(o, J, J_new, dV1, dV2, alpha):
    """One iLQR trial: (delta_J, ratio, accepted)."""
    delta_J = J - J_new
    ratio = _ratio(delta_J, -alpha * (dV1 + alpha * dV2))
    return delta_J, ratio, bool(ratio >= o["expected_reduction_min_SQP_DDP"]
                                and ratio <= o["expected_reduction_max_SQP_DDP"])


def step_outcome(o, error, delta_J, it, rho, drho):
    """Iteration `it` after its line search (error: nothing accepted).  Returns (trace_rho, rho, drho, exit_code,
    it): rho reduced on success -- the value the trace row records -- and grown on error; exit 2 / 1 / 3 (the
    last iteration, which overrides them) / 0 (go on); the next iteration's number."""
    f = o["rho_factor_SQP_DDP"]
    if not error:
        drho = min(drho / f, 1 / f)
        rho = max(rho * drho, o["rho_min_SQP_DDP"])
    trace_rho = rho
    exit_code = 0
    if error:
        drho = max(drho * f, f)
        rho = max(rho * drho, o["rho_min_SQP_DDP"])
        if rho > o["rho_max_SQP_DDP"]:
            exit_code = 2
    elif delta_J < o["exit_tolerance_SQP_DDP"]:
        exit_code = 1
    if it == o["max_iter_SQP_DDP"] - 1:
        exit_code = 3
    else:
        it += 1
    return trace_rho, rho, drho, exit_code, it


def outer_exit(o, max_c, outer):
    """check_and_update_soft_constraints' exit rule before the constants' update: (exit_soft, outer) with exit 1
    (max_c below the tolerance) / 2 (the last outer iteration, which overrides it) / 0 (update and go on, or
    exit 3 when the update changes nothing)."""
    exit_soft = 1 if max_c < o["exit_tolerance_softConstraints"] else 0
    if outer == o["max_iter_softConstraints"] - 1:
        exit_soft = 2
    else:
        outer += 1
    return exit_soft, outer
