"""The SQP's line search (k_ls_terms: its dense cost value, the C->diag == 0 branch and the directional
derivative D) and whole solves on dense costs, in the replay style of the suite: nothing is compared between
two runs whose S differ by rounding.

Shapes: arm3 N = 8, arm6 N = 16, arm12 N = 4, B = 8, PCG-SS and S, dense Q, QF, R and a non-zero goal
(ilqr_cases.cost_arrays("dense")), arm3 once with a dense QF_start, and arm6 once with augmented-Lagrangian
torque limits at +-0.02 (one outer pass, so every QP and trial sees the limits' initial constants; the soft
values and jacobians enter J and D).

Per iteration j of the GPU's own run and per problem: the iterate is the same solve stopped after j iterations,
dxul comes from tmpc_qp_batch at the trace's rho_j, and osqp.line_search from that iterate with that dxul must
return the trace's alpha, line_search_iteration and acceptance.  The one exception is test_gpu_ilqr._replay's: a
decision taken at the rounding floor of the merit (the oracle's merit at the trial where the two part differs
from the current merit by at most 1e-12 of it); at most 1 in 8 decisions may claim it.  J, c and merit of the
iterate (trace row j) and of the accepted trial (row j + 1) must be the oracle's evaluations within LS_BOUND.
Whole run: exit code and iteration count are those conftest.derived_exit derives from the run's own trace, and
conftest.replay_qp_counts holds for the first two problems of each PCG case (every QP's count and lambda through
oracle/canon.c; it re-solves once per QP, so two problems keep a case within a few seconds).
Not here: the comparison of final x, u with the oracle's whole run on the problems both sides converge on: from these
starts (seeds 1200..1207) every oracle run on the dense cost ends with exit 2 after 5..17 iterations, all three
shapes and both methods, as the GPU's do -- rho runs past rho_max, the usual end of this workload -- so there is
no converged problem to compare, and 8 oracle solves of arm12 or arm6 take 3..5 s.
MEASURED on the MI355X: 421 decisions over the eight cases (65 with the torque limits, violated at 16 knots or
more), all identical to the oracle's, none at the rounding floor; the largest J / c / merit deviation is LS_MEASURED.
"""
import warnings

import numpy as np
import pytest

import qp_cases as qc
from conftest import derived_exit, replay_qp_counts
from oracle import sqp as osqp
from oracle.soft import SoftConstraints, SoftLimit

pytestmark = pytest.mark.gpu

DT = 0.1
# largest deviation of a trace row's J, c, merit from the oracle's evaluation at the same point, relative to
# max(1, |ref|), measured on the MI355X for this test; the bound is 8 x that, at most 1e-10 (identical inputs: one
# evaluation, not a solve)
LS_MEASURED = 3.06e-14   # arm12 N = 4 PCG-SS; arm6 N = 16 1.8e-14, arm3 N = 8 2.2e-15, torque AL 1.2e-14
LS_BOUND = min(8 * LS_MEASURED, 1e-10)
FLOOR = 1e-12

CASES = [(key, N, "dense", method, False) for key, N in (("arm3", 8), ("arm6", 16), ("arm12", 4))
         for method in ("PCG-SS", "S")] + [("arm3", 8, "qfstart-dense", "PCG-SS", False),
                                           ("arm6", 16, "dense", "PCG-SS", True)]
TORQUE_BOUND = 0.02   # the augmented-Lagrangian torque limits of the soft case: +-0.02


def _solver(key, N, cost, soft):
    from trajoptmpcreference_amd import (QuadraticCost, TrajoptConstraint, TrajoptMPCReference, URDFPlant,
                                         planar_arm_urdf)
    n = qc.model(key).n
    con = None
    if soft:
        con = TrajoptConstraint(n, n, n, N)
        con.set_torque_limits([TORQUE_BOUND] * n, [-TORQUE_BOUND] * n, "AUGMENTED_LAGRANGIAN")
    return TrajoptMPCReference(URDFPlant(options={"path_to_urdf": planar_arm_urdf(n)}),
                               QuadraticCost(*qc.cost_arrays(cost, n, N)), con)


def _soft_oracle(n, N, soft):
    """the oracle's torque limits at their initial constants (the one outer pass the soft case runs)"""
    if not soft:
        return None
    return SoftConstraints([SoftLimit("torque", n, N, [-TORQUE_BOUND] * n, [TORQUE_BOUND] * n,
                                      "AUGMENTED_LAGRANGIAN")])


def _rows(r, i):
    """problem i's trace rows as dicts: the initial row and one per QP"""
    nq = int(r["sqp_iter"][i]) + (1 if int(r["exit_sqp"][i]) == 3 else 0)
    t = r["trace"]
    return [{k: t[k][i, q] for k in ("J", "c", "merit", "alpha", "line_search_iteration", "succeeded_line_search",
                                     "pcg_iters")} for q in range(nq + 1)]


def _dev(a, ref):
    return abs(float(a) - float(ref)) / max(1.0, abs(float(ref)))


@pytest.mark.parametrize("key,N,cost,method,soft", CASES,
                         ids=[f"{c[0]}-N{c[1]}-{c[2]}-{c[3]}{'-torque-al' if c[4] else ''}" for c in CASES])
def test_dense_cost_solve_replays_through_the_oracle(key, N, cost, method, soft):
    m = qc.model(key)
    n, nx, B = m.n, 2 * m.n, 8
    oc = osqp.QuadCost(*qc.cost_arrays(cost, n, N))
    solver = _solver(key, N, cost, soft)
    # the soft case runs one outer pass: every QP and line search sees the limits' initial constants
    base = {"max_iter_softConstraints": 1} if soft else {}
    violated = 0
    probs = [osqp.initial_problem(m, N, DT, 1200 + i) for i in range(B)]
    x0, u0 = np.array([p[0] for p in probs]), np.array([p[1] for p in probs])
    r = solver.SQP_batch(x0, u0, N, DT, method, dict(base))
    opts = dict(base)
    solver.set_default_options(opts)
    o = osqp.default_options()
    rows = [_rows(r, i) for i in range(B)]
    f, mu = float(o["rho_factor_SQP_DDP"]), 10
    worst, decisions, floor_claims = 0.0, 0, []
    for j in range(max(len(t) for t in rows) - 1):
        live = [i for i in range(B) if j + 1 < len(rows[i])]
        if j == 0:
            xj, uj = x0, u0
        else:   # the GPU's own iterate j: the same solve stopped after j iterations
            rj = solver.SQP_batch(x0, u0, N, DT, method, dict(base, max_iter_SQP_DDP=j))
            xj, uj = rj["x"], rj["u"]
        rho = np.zeros(B)
        for i in range(B):   # rho_j from the trace's schedule (check_for_exit_or_error :463-481)
            rh, drho = o["rho_init_SQP_DDP"], 1.0
            for q in range(min(j, len(rows[i]) - 1)):
                drho = min(drho / f, 1.0 / f) if rows[i][q + 1]["succeeded_line_search"] else max(drho * f, f)
                rh = max(rh * drho, o["rho_min_SQP_DDP"])
            rho[i] = rh
        ctx = solver._context(dict(opts))
        if soft:
            ctx.set_soft_state(B, N)   # the initial constants, right before the call (include/tmpc.h)
        q = ctx.qp_batch(xj, uj, N, DT, rho, method, want_blocks=False, xs=x0[:, :, 0])
        for i in live:
            row, nxt = rows[i][j], rows[i][j + 1]
            xs = x0[i][:, 0]
            so = _soft_oracle(n, N, soft)
            violated += int(np.sum(np.any(np.abs(uj[i]) > TORQUE_BOUND, axis=0))) if soft else 0
            J0 = osqp.total_cost(oc, xj[i], uj[i], N, so)
            c0 = osqp.total_violation(m, xj[i], uj[i], xs, N, DT)
            merit0 = J0 + mu * c0
            d0 = max(_dev(row["J"], J0), _dev(row["c"], c0), _dev(row["merit"], merit0))
            ls = osqp.line_search(oc, m, xj[i], uj[i], xs, N, DT, q["dxul"][i], J0, merit0, mu, o, soft=so)
            decisions += 1
            same = (int(nxt["line_search_iteration"]), float(nxt["alpha"]), bool(nxt["succeeded_line_search"])) == \
                (ls["ls"], float(ls["alpha"]), bool(ls["succeeded_line_search"]))
            worst = max(worst, d0)
            print(f"{key} N={N} {cost} {method} problem {i} QP {j}: iterate deviation {d0:.2e}, "
                  f"alpha {float(nxt['alpha'])} ls {int(nxt['line_search_iteration'])} "
                  f"ok {bool(nxt['succeeded_line_search'])} same {same}")
            assert d0 <= LS_BOUND, (i, j, d0)
            if not same:
                # only at the rounding floor of the merit: the oracle's returned trial and the GPU's row both sit
                # within 1e-12 of the current merit
                fl = FLOOR * max(1.0, abs(merit0))
                assert abs(ls["merit"] - merit0) <= fl and abs(float(nxt["merit"]) - merit0) <= fl, \
                    (i, j, "decision differs above the rounding floor", ls["merit"], float(nxt["merit"]), merit0)
                floor_claims.append((i, j))
                continue
            if ls["succeeded_line_search"]:
                d1 = max(_dev(nxt["J"], ls["J"]), _dev(nxt["c"], ls["c"]), _dev(nxt["merit"], ls["merit"]))
                worst = max(worst, d1)
                assert d1 <= LS_BOUND, (i, j, d1)
    assert 8 * len(floor_claims) <= decisions, (floor_claims, decisions)
    assert not soft or violated >= 2 * B, ("the torque limits are hardly ever violated", violated)
    warnings.warn(f"{key} N={N} {cost} {method}: {decisions} decisions, {len(floor_claims)} at the rounding floor, "
                  f"largest J / c / merit deviation {worst:.3g}")
    for i in range(B):
        assert (int(r["exit_sqp"][i]), int(r["sqp_iter"][i])) == derived_exit(rows[i], opts), i
        if method.startswith("PCG") and i < 2 and not soft:   # every QP's PCG count and lambda through canon.c
            replay_qp_counts(solver, x0[i:i + 1], u0[i:i + 1], N, DT, method,
                             [int(t["pcg_iters"]) for t in rows[i][1:]],
                             [bool(t["succeeded_line_search"]) for t in rows[i][1:]])
