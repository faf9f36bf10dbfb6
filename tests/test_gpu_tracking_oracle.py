"""GPU parity of tracking solves (per-knot references: TrackingCost / goal=, tmpc_set_reference) against the
oracle, which is duck-typed on cost.value / gradient / hessian(..., k) and takes tracking_cases.TrackCost
unchanged.  The comparisons and bounds are those of the fixed-goal suites: test_gpu_sqp.py (integers identical,
J / c / merit and trajectories at 1e-7, every later QP's PCG count through conftest.replay_qp_counts),
test_gpu_ilqr.py (_replay with its rounding-floor rule, _check_full), test_gpu_soft.py / test_gpu_hard.py,
test_gpu_mpc.py (per-step integers identical, executed states / controls at 1e-6) and test_gpu_precision.py.

oracle/mpc.py has no hook to slide a reference, so the MPC test restates its loop and sets cost.step per step.
"""
import warnings

import numpy as np
import pytest

from conftest import arm_model, replay_qp_counts
from tracking_cases import fixed_solver, oracle_cost, reference, tracking_solver

pytestmark = pytest.mark.gpu

DT = 0.1
SHAPES = [("arm2", 4), ("arm3", 8), ("arm3", 16), ("arm6fix", 8)]
SEEDS = (0, 1)


def _start(name, N, seed):
    from oracle import sqp as osqp
    return osqp.initial_problem(arm_model(name), N, DT, seed)


@pytest.mark.parametrize("method", ["PCG-SS", "S"])
@pytest.mark.parametrize("extra", [0, 3], ids=["M=N", "M=N+3"])
@pytest.mark.parametrize("name,N", SHAPES, ids=[f"{a}-N{b}" for a, b in SHAPES])
def test_sqp_per_knot_reference_matches_oracle(name, N, extra, method):
    from oracle import sqp as osqp
    m = arm_model(name)
    for seed in SEEDS:
        xref = reference(m.n, N + extra, seed)
        x0, u0 = _start(name, N, seed)
        solver = tracking_solver(name, xref)
        x, u, exit_sqp, exit_soft, outer_iter, sqp_iter = solver.SQP(x0, u0, N, DT, method, {})
        o = osqp.sqp(m, oracle_cost(m.n, xref), x0, u0, N, DT, method)
        assert (exit_sqp, exit_soft, outer_iter, sqp_iter) == (o["exit_sqp"], o["exit_soft"], o["outer_iter"],
                                                               o["sqp_iter"]), seed
        tr, otr = solver.trace, o["trace"]
        assert len(tr) == len(otr)
        for key in ("alpha", "line_search_iteration", "succeeded_line_search"):
            assert [t[key] for t in tr] == [t[key] for t in otr], (seed, key)
        for key in ("J", "c", "merit", "rho"):
            assert np.allclose([t[key] for t in tr], [t[key] for t in otr], rtol=1e-7, atol=1e-12), (seed, key)
        for a, b in ((x, o["x"]), (u, o["u"])):
            assert float(np.max(np.abs(a - b))) < 1e-7 * max(1.0, float(np.max(np.abs(b)))), seed
        ours = [t["inner_iters"] for t in tr[1:]]
        if method == "S":
            assert ours == [0] * len(ours)
        else:
            assert ours[0] == o["pcg_iters"][0], seed   # QP 0: identical inputs
            replay_qp_counts(solver, x0[None], u0[None], N, DT, method, ours,
                             [t["succeeded_line_search"] for t in tr[1:]])


ILQR_CASES = [("arm2", 4, 0), ("arm2", 4, 3), ("arm3", 8, 0), ("arm3", 8, 3), ("arm3", 16, 0), ("arm3", 16, 3),
              ("arm6fix", 8, 3), ("arm6fix", 8, None)]   # arm6fix: M = N + 3 and M = 1 (the oracle's M = N runs
                                                         # take up to 91 iterations)


@pytest.mark.parametrize("name,N,extra", ILQR_CASES,
                         ids=[f"{a}-N{b}-M={'1' if c is None else 'N+' + str(c)}" for a, b, c in ILQR_CASES])
def test_ilqr_per_knot_reference_matches_oracle(name, N, extra):
    from oracle import ilqr as oilqr
    from test_gpu_ilqr import _check_full, _replay
    m = arm_model(name)
    for seed in SEEDS:
        xref = reference(m.n, 1 if extra is None else N + extra, seed)
        x0, u0 = _start(name, N, seed)
        solver = tracking_solver(name, xref)
        r = solver.iLQR_batch(x0[None], u0[None], N, DT, {})
        cost = oracle_cost(m.n, xref)
        with np.errstate(all="ignore"):
            _check_full(r, 0, oilqr.ilqr(m, cost, x0, u0, N, DT, {}))
        _replay(solver, r, m, cost, x0[None], u0[None], N)


# ------------------------------------------------------------------ limits (arm3 N = 8, per-knot reference)
def _limits(n, N, spec):
    from trajoptmpcreference_amd import TrajoptConstraint
    con = TrajoptConstraint(n, n, n, N)
    for kind, (lb, ub, mode) in spec.items():
        getattr(con, f"set_{kind}_limits")([ub] * n, [lb] * n, mode)
    return con


# Torque bounds +-2.0: the unconstrained tracking optima of these problems reach |u| = 4.7 / 3.6 (seeds 0 / 1), so the
# limits are active; at test_gpu_soft.py's +-0.7 the oracle's own SQP run of seed 0 diverges to NaN and raises
# (np.linalg.inv of a non-finite block), so that bound has no reference to compare with.
SOFT_BOUND = 2.0


def test_al_torque_limits_under_sqp_match_oracle():
    """test_gpu_soft.py's assertions: the four integers identical, x at 1e-6, mu bitwise."""
    from oracle import sqp as osqp
    from oracle.soft import SoftConstraints, SoftLimit
    name, n, N = "arm3", 3, 8
    m = arm_model(name)
    spec = {"torque": (-SOFT_BOUND, SOFT_BOUND, "AUGMENTED_LAGRANGIAN")}
    for seed in SEEDS:
        xref = reference(n, N, seed)
        x0, u0 = _start(name, N, seed)
        solver = tracking_solver(name, xref, _limits(n, N, spec))
        r = solver.SQP_batch(x0[None], u0[None], N, DT, "PCG-SS", {})
        lim = SoftLimit("torque", n, N, [-SOFT_BOUND] * n, [SOFT_BOUND] * n, "AUGMENTED_LAGRANGIAN")
        o = osqp.sqp(m, oracle_cost(n, xref), x0, u0, N, DT, "PCG-SS", {}, SoftConstraints([lim]))
        got = (int(r["exit_sqp"][0]), int(r["exit_soft"][0]), int(r["outer_iter"][0]), int(r["sqp_iter"][0]))
        assert got == (o["exit_sqp"], o["exit_soft"], o["outer_iter"], o["sqp_iter"]), (seed, got)
        assert float(np.max(np.abs(r["x"][0] - o["x"]))) < 1e-6 * max(1.0, float(np.max(np.abs(o["x"])))), seed
        assert np.array_equal(r["soft_state"][0][0, :lim.T, 4 * n:6 * n].T, lim.mu), seed


def test_al_torque_limits_under_ilqr_match_oracle():
    """test_gpu_ilqr.py's soft-limit assertions: the four integers and the last pass's alpha path identical, the
    final cost / trajectory by _check_full, mu bitwise.  3 outer passes of at most 10 iterations: the oracle's
    default-option run of these problems takes 20-36 s on the CPU."""
    from oracle import ilqr as oilqr
    from oracle.soft import SoftConstraints, SoftLimit
    from test_gpu_ilqr import _check_full, _key
    name, n, N = "arm3", 3, 8
    m = arm_model(name)
    spec = {"torque": (-SOFT_BOUND, SOFT_BOUND, "AUGMENTED_LAGRANGIAN")}
    for seed in SEEDS:
        xref = reference(n, N, seed)
        x0, u0 = _start(name, N, seed)
        solver = tracking_solver(name, xref, _limits(n, N, spec))
        opts = {"max_iter_SQP_DDP": 10, "max_iter_softConstraints": 3}
        r = solver.iLQR_batch(x0[None], u0[None], N, DT, dict(opts))
        lim = SoftLimit("torque", n, N, [-SOFT_BOUND] * n, [SOFT_BOUND] * n, "AUGMENTED_LAGRANGIAN")
        with np.errstate(all="ignore"):
            o = oilqr.ilqr(m, oracle_cost(n, xref), x0, u0, N, DT, dict(opts), SoftConstraints([lim]))
        got = (int(r["exit_code"][0]), int(r["iter"][0]), int(r["exit_soft"][0]), int(r["outer_iter"][0]))
        assert got == _key(o), (seed, got, _key(o))
        rows = len(o["trace"])
        assert list(r["trace"]["alpha"][0, 1:rows]) == [t["alpha"] for t in o["trace"][1:]], seed
        _check_full(r, 0, o)
        assert np.array_equal(r["soft_state"][0][0, :lim.T, 4 * n:6 * n].T, lim.mu), seed


def test_active_set_torque_limits_under_sqp_match_oracle():
    """The banded QP's gradient site (tmpc_hard.hip): test_gpu_hard.py's assertions against the canonical-order
    oracle -- exit code, iterations, alpha path, every QP's active set and singular flag identical, x at 1e-5.

    Bounds +-2.0 (active: the masks are asserted non-empty).  The comparison needs QPs whose PCG converges in the
    oracle's own run, which the test asserts on the oracle alone: at +-0.3 the oracle's QPs 2 and 3 of seed 0 take
    97 and 100 = max_iter_linSys iterations, i.e. lambda is an unconverged iterate that the last bits of S decide
    (test_gpu_hard.py's docstring describes the same on its systems), and the two runs part there -- measured on
    the MI355X: rows 0-1 agree to 1e-12, row 2 (97 iterations both) has c = 19.6658 against 19.6596, after which
    the GPU exits at iteration 8 and the oracle at 9; seed 1 at +-0.3 and both seeds at +-2.0 agree in every
    integer.  A constant reference under these limits is bitwise the fixed-goal solve (asserted below), which pins
    the gradient site itself."""
    from oracle import hard as ohard
    from oracle import sqp as osqp
    name, n, N = "arm3", 3, 8
    m = arm_model(name)
    spec = {"torque": (-SOFT_BOUND, SOFT_BOUND, "ACTIVE_SET")}
    hard = ohard.HardConstraints([ohard.HardLimit(k, n, lb, ub, mode) for k, (lb, ub, mode) in spec.items()])
    for seed in SEEDS:
        xref = reference(n, N, seed)
        x0, u0 = _start(name, N, seed)
        solver = tracking_solver(name, xref, _limits(n, N, spec))
        r = solver.SQP_batch(x0[None], u0[None], N, DT, "PCG-SS", {}, hard_active=True)
        o = osqp.sqp(m, oracle_cost(n, xref), x0, u0, N, DT, "PCG-SS", {}, hard=hard, order="canonical")
        assert max(o["pcg_iters"]) < 100, "an oracle QP ran into max_iter_linSys: its step is rounding-decided"
        got = (int(r["exit_sqp"][0]), int(r["sqp_iter"][0]))
        assert got == (o["exit_sqp"], o["sqp_iter"]), (seed, got)
        nq = got[1] + (1 if got[0] == 3 else 0)
        assert list(r["trace"]["alpha"][0, 1:nq + 1]) == [t["alpha"] for t in o["trace"][1:]], seed
        masks = [[int(v) for v in r["trace"]["hard_active"][0, q + 1]] for q in range(nq)]
        assert masks == o["active_masks"], seed
        assert any(any(row) for row in masks), "the limits never became active: the case checks nothing"
        assert [bool(v) for v in r["trace"]["singular"][0, 1:nq + 1]] == o["singular"], seed
        assert float(np.max(np.abs(r["x"][0] - o["x"]))) < 1e-5 * max(1.0, float(np.max(np.abs(o["x"])))), seed


def test_constant_reference_under_hard_limits_is_the_fixed_goal_bitwise():
    name, n, N = "arm3", 3, 8
    xg = np.random.default_rng(7).uniform(-0.5, 0.5, 2 * n)
    x0, u0 = _start(name, N, 0)
    f = fixed_solver(name, xg, _limits(n, N, {"torque": (-0.3, 0.3, "ACTIVE_SET")}))
    a = f.SQP_batch(x0[None], u0[None], N, DT, "PCG-SS", {})
    b = f.SQP_batch(x0[None], u0[None], N, DT, "PCG-SS", {}, goal=np.broadcast_to(xg[None, :, None], (1, 2 * n, N)))
    assert int(a["sqp_iter"][0]) > 1
    for k in ("x", "u", "exit_sqp", "sqp_iter"):
        assert np.array_equal(a[k], b[k]), k


# ------------------------------------------------------------------ MPC
def _oracle_mpc(m, cost, x, u, N, method, steps, options):
    """oracle/mpc.py's loop with the reference sliding one column per step (cost.step = s)."""
    from oracle import ilqr as oilqr
    from oracle import rbd
    from oracle import sqp as osqp
    x, u = np.array(x, dtype=float), np.array(u, dtype=float)
    xe, ue = np.zeros((x.shape[0], steps + 1)), np.zeros((u.shape[0], steps))
    codes, iters = np.zeros(steps, dtype=np.int64), np.zeros(steps, dtype=np.int64)
    xe[:, 0] = x[:, 0]
    for s in range(steps):
        cost.step = s
        if method == "iLQR":
            r = oilqr.ilqr(m, cost, x, u, N, DT, options)
            codes[s], iters[s] = r["exit_code"], r["iter"]
        else:
            r = osqp.sqp(m, cost, x, u, N, DT, method, options)
            codes[s], iters[s] = r["exit_sqp"], r["sqp_iter"]
        x, u = r["x"], r["u"]
        x_next = rbd.euler(m, x[:, 0][None], u[:, 0][None], DT)[0]
        ue[:, s], xe[:, s + 1] = u[:, 0], x_next
        x = np.concatenate([x[:, 1:], x[:, -1:]], axis=1)
        u = np.concatenate([u[:, 1:], u[:, -1:]], axis=1)
        x[:, 0] = x_next
    return dict(x_exec=xe, u_exec=ue, exit_codes=codes, iters=iters, x=x, u=u)


@pytest.mark.parametrize("method", ["QP-PCG-SS", "iLQR"])
def test_mpc_tracks_a_sliding_reference_like_the_oracle(method):
    name, n, N, B, steps = "arm3", 3, 8, 3, 3
    m = arm_model(name)
    refs = np.array([reference(n, N + 2, s) for s in range(B)])
    xs, us = zip(*[_start(name, N, s) for s in range(B)])
    opts = {"max_iter_SQP_DDP": 8}
    r = fixed_solver(name).MPC_batch(np.array(xs), np.array(us), N, DT, method, dict(opts), mpc_steps=steps, goal=refs)
    for i in range(B):
        with np.errstate(all="ignore"):
            o = _oracle_mpc(m, oracle_cost(n, refs[i]), xs[i], us[i], N, "iLQR" if method == "iLQR" else method[3:],
                            steps, dict(opts))
        assert list(r["exit_codes"][i]) == list(o["exit_codes"]), i
        assert list(r["iters"][i]) == list(o["iters"]), i
        assert np.allclose(r["x_exec"][i], o["x_exec"], rtol=1e-6, atol=1e-8), i
        assert np.allclose(r["u_exec"][i], o["u_exec"], rtol=1e-6, atol=1e-8), i


# ------------------------------------------------------------------ precision modes
def _rel(a, b):
    return float(np.max(np.abs(np.asarray(a) - np.asarray(b)))) / max(1.0, float(np.max(np.abs(b))))


@pytest.fixture
def fp64_afterwards():
    """the precision mode is an option of the shared per-device context: put fp64 back for whoever uses it next"""
    yield
    s = fixed_solver("arm3")
    o = {}
    s.set_default_options(o)
    s._context(o)


def test_fp32_ilqr_tracks_the_fp64_oracle(fp64_afterwards):
    """test_gpu_precision.py's iLQR bounds (fp32): states within 3e-3 relative of the fp64 result, controls
    within 2e-2; exit codes are not compared there (the exit test is below fp32 rounding).  Here the fp64
    result is the oracle's."""
    from oracle import ilqr as oilqr
    name, n, N = "arm3", 3, 8
    m = arm_model(name)
    ex, eu = [], []
    for seed in SEEDS:
        xref = reference(n, N, seed)
        x0, u0 = _start(name, N, seed)
        r = tracking_solver(name, xref).iLQR_batch(x0[None], u0[None], N, DT, {"precision": "fp32"})
        with np.errstate(all="ignore"):
            o = oilqr.ilqr(m, oracle_cost(n, xref), x0, u0, N, DT, {})
        ex.append(_rel(r["x"][0], o["x"]))
        eu.append(_rel(r["u"][0], o["u"]))
    warnings.warn(f"fp32 tracking iLQR arm3 N=8: max rel err vs the fp64 oracle x {max(ex):.2e} (bound 3e-3), "
                  f"u {max(eu):.2e} (bound 2e-2)")
    print("fp32 tracking iLQR", ex, eu)
    assert max(ex) < 3e-3, ex
    assert max(eu) < 2e-2, eu


def test_mixed_sqp_tracks_the_fp64_oracle(fp64_afterwards):
    """test_gpu_precision.py's SQP PCG-SS bound for the mixed mode (its config-5 check): exit codes and SQP
    iterations identical to the fp64 oracle, states within 1e-4."""
    from oracle import sqp as osqp
    name, n, N = "arm3", 3, 8
    m = arm_model(name)
    errs = []
    for seed in SEEDS:
        xref = reference(n, N, seed)
        x0, u0 = _start(name, N, seed)
        r = tracking_solver(name, xref).SQP_batch(x0[None], u0[None], N, DT, "PCG-SS", {"precision": "mixed"})
        o = osqp.sqp(m, oracle_cost(n, xref), x0, u0, N, DT, "PCG-SS")
        assert (int(r["exit_sqp"][0]), int(r["sqp_iter"][0])) == (o["exit_sqp"], o["sqp_iter"]), seed
        errs.append(_rel(r["x"][0], o["x"]))
    warnings.warn(f"mixed tracking SQP arm3 N=8: max state rel err vs the fp64 oracle {max(errs):.2e} (bound 1e-4)")
    print("mixed tracking SQP", errs)
    assert max(errs) < 1e-4, errs
