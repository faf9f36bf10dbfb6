"""GPU: per-problem goals and per-knot references (goal=, TrackingCost, tmpc_set_reference) -- the properties that
hold bit for bit.  A reference whose columns all equal the cost's xg is the fixed-goal solve; row p of a batch with
per-problem goals is the single solve of a QuadraticCost with that goal; a stream's problems are the batch's; a
reference that runs out in the MPC loop is the same reference padded with its last column; and a goal leaves
nothing behind in the shared context.  (Against the oracle: test_gpu_tracking_oracle.py.)"""
import numpy as np
import pytest

from conftest import quad_cost_arrays
from tracking_cases import fixed_solver, reference, tracking_solver

pytestmark = pytest.mark.gpu

DT = 0.1


def _problems(n, N, B, seed=0):
    from oracle import sqp as osqp
    from trajoptmpcreference_amd.urdf import parse_urdf, planar_arm_urdf
    m = parse_urdf(planar_arm_urdf(n))
    xs, us = zip(*[osqp.initial_problem(m, N, DT, seed + i) for i in range(B)])
    return np.array(xs), np.array(us)


def _solver_n(n, xg=None):
    from trajoptmpcreference_amd import QuadraticCost, TrajoptMPCReference, URDFPlant, planar_arm_urdf
    Q, QF, R, z = quad_cost_arrays(n)
    return TrajoptMPCReference(URDFPlant(options={"path_to_urdf": planar_arm_urdf(n)}),
                               QuadraticCost(Q, QF, R, z if xg is None else xg))


def _same(a, b):
    """every array of two result dicts, bit for bit; of the trace the rows the solve wrote (the initial row and
    one per iteration -- the rows past them are whatever the buffer held)"""
    assert a.keys() == b.keys()
    for k in a:
        if k == "trace":
            it = a["iter" if "iter" in a else "sqp_iter"]
            code = a["exit_code" if "exit_code" in a else "exit_sqp"]
            assert a[k].keys() == b[k].keys()
            for f in a[k]:
                for i in range(len(it)):
                    rows = min(int(it[i]) + 1 + (int(code[i]) == 3), a[k][f].shape[1])
                    assert np.array_equal(a[k][f][i, :rows], b[k][f][i, :rows], equal_nan=True), (f, i)
        elif isinstance(a[k], tuple):
            for p, q in zip(a[k], b[k]):
                assert np.array_equal(p, q, equal_nan=True), k
        else:
            assert np.array_equal(a[k], b[k], equal_nan=True), k


def _run(solver, which, x, u, N, **kw):
    if which == "iLQR":
        return solver.iLQR_batch(x, u, N, DT, {}, **kw)
    return solver.SQP_batch(x, u, N, DT, which, {}, **kw)


@pytest.mark.parametrize("which", ["PCG-SS", "S", "iLQR"])
def test_constant_reference_is_the_fixed_goal_bitwise(which):
    n, N, B = 3, 8, 4
    xg = np.random.default_rng(7).uniform(-0.5, 0.5, 2 * n)   # a non-zero goal: x - xg rounds
    solver = _solver_n(n, xg)
    x, u = _problems(n, N, B)
    base = _run(solver, which, x, u, N)
    _same(base, _run(solver, which, x, u, N, goal=np.broadcast_to(xg, (B, 2 * n))))
    _same(base, _run(solver, which, x, u, N, goal=np.broadcast_to(xg[None, :, None], (B, 2 * n, N))))
    _same(base, _run(solver, which, x, u, N, goal=xg[None, :, None]))          # one row for every problem
    _same(base, _run(solver, which, x, u, N))                                   # and nothing is left behind


@pytest.mark.parametrize("n,N", [(3, 8), (6, 8), (8, 4)], ids=["arm3-N8", "arm6-N8", "arm8-N4-runtime-model"])
@pytest.mark.parametrize("which", ["PCG-SS", "iLQR"])
def test_per_problem_goals_index_the_right_problem(n, N, which):
    B = 5
    goals = np.random.default_rng(11).uniform(-0.6, 0.6, (B, 2 * n))
    x, u = _problems(n, N, B, seed=20)
    r = _run(_solver_n(n), which, x, u, N, goal=goals)
    for i in range(B):
        one = _solver_n(n, goals[i])
        if which == "iLQR":
            xi, ui, code, _, _, it = one.iLQR(x[i], u[i], N, DT, {})
            assert (code, it) == (int(r["exit_code"][i]), int(r["iter"][i])), i
        else:
            xi, ui, code, _, _, it = one.SQP(x[i], u[i], N, DT, which, {})
            assert (code, it) == (int(r["exit_sqp"][i]), int(r["sqp_iter"][i])), i
        assert np.array_equal(r["x"][i], xi), i
        assert np.array_equal(r["u"][i], ui), i


@pytest.mark.parametrize("solver_name", ["PCG-SS", "iLQR"])
@pytest.mark.parametrize("substreams", [1, 2])
def test_stream_equals_batch_bitwise(solver_name, substreams):
    """12 problems through 4 slots (handover), period 6 (the % of the reference row and of the inputs)."""
    n, N, period, copies, slots = 3, 8, 6, 2, 4
    x, u = _problems(n, N, period, seed=40)
    refs = np.array([reference(n, N, s) for s in range(period)])
    solver = _solver_n(n)
    P = period * copies
    xb, ub = np.tile(x, (copies, 1, 1)), np.tile(u, (copies, 1, 1))
    batch = _run(solver, solver_name, xb, ub, N, goal=np.tile(refs, (copies, 1, 1)))
    opts = {}
    solver.set_default_options(opts)
    ctx = solver._context(opts)
    st = ctx.solve_stream(x, u, N, DT, solver=solver_name, slots=slots, copies=copies, substreams=substreams,
                          goal=refs)
    codes = batch["exit_code" if solver_name == "iLQR" else "exit_sqp"]
    iters = batch["iter" if solver_name == "iLQR" else "sqp_iter"]
    assert st["x"].shape[0] == P
    assert np.array_equal(st["x"], batch["x"])
    assert np.array_equal(st["u"], batch["u"])
    assert np.array_equal(st["exit"], codes) and np.array_equal(st["iters"], iters)
    # the stream left no reference in the shared context, and the references changed the solves at all
    assert not np.array_equal(batch["x"], _run(solver, solver_name, xb, ub, N)["x"])


@pytest.mark.parametrize("method", ["QP-PCG-SS", "iLQR"])
def test_mpc_reference_holds_its_last_column(method):
    """M = N: the window runs out after step 0; it must be the reference padded by its last column."""
    n, N, B, steps = 3, 8, 3, 3
    x, u = _problems(n, N, B, seed=60)
    refs = np.array([reference(n, N, s) for s in range(B)])
    padded = np.concatenate([refs, np.repeat(refs[:, :, -1:], steps - 1, axis=2)], axis=2)
    solver = _solver_n(n)
    opts = {"max_iter_SQP_DDP": 8}
    a = solver.MPC_batch(x, u, N, DT, method, dict(opts), mpc_steps=steps, goal=refs)
    b = solver.MPC_batch(x, u, N, DT, method, dict(opts), mpc_steps=steps, goal=padded)
    _same(a, b)


def test_tracking_cost_through_mpc_advances_its_shift():
    n, N, steps = 3, 8, 3
    x, u = _problems(n, N, 1, seed=70)
    xref = reference(n, N + 2, 1)
    s = tracking_solver("arm3", xref)
    xe, ue, codes, iters = s.MPC(x[0], u[0], N, DT, "QP-PCG-SS", {"max_iter_SQP_DDP": 8}, mpc_steps=steps)
    assert s.cost.shift == steps
    r = fixed_solver("arm3").MPC_batch(x, u, N, DT, "QP-PCG-SS", {"max_iter_SQP_DDP": 8}, mpc_steps=steps,
                                       goal=xref[None])
    assert np.array_equal(xe, r["x_exec"][0]) and np.array_equal(ue, r["u_exec"][0])
    # goal= replaces the cost's reference for the call: the loop never tracked the cost's own, whose shift stays
    s.MPC_batch(x, u, N, DT, "QP-PCG-SS", {"max_iter_SQP_DDP": 8}, mpc_steps=2, goal=xref[None])
    assert s.cost.shift == steps
    # the next call goes on from the shifted reference
    s2 = tracking_solver("arm3", xref[:, steps:])
    a = s.SQP(x[0], u[0], N, DT, "PCG-SS", {})
    b = s2.SQP(x[0], u[0], N, DT, "PCG-SS", {})
    assert np.array_equal(a[0], b[0]) and a[2:] == b[2:]


def test_no_reference_outlives_its_call():
    n, N, B = 3, 8, 4
    x, u = _problems(n, N, B, seed=80)
    solver = _solver_n(n)
    base = _run(solver, "PCG-SS", x, u, N)
    goals = np.random.default_rng(3).uniform(-0.5, 0.5, (B, 2 * n))
    moved = _run(solver, "PCG-SS", x, u, N, goal=goals)
    assert not np.array_equal(moved["x"], base["x"])
    # the solver cleared it after its solve: a direct user of the shared context sees none
    direct = solver.plant._ctx().sqp_solve_batch(x, u, N, DT, "PCG-SS")
    assert np.array_equal(direct["x"], base["x"]) and np.array_equal(direct["sqp_iter"], base["sqp_iter"])
    _same(base, _run(solver, "PCG-SS", x, u, N))
    _same(base, _run(_solver_n(n), "PCG-SS", x, u, N))   # another solver object on the same shared context
    # tmpc_set_model after tmpc_set_reference leaves no reference behind
    opts = {}
    solver.set_default_options(opts)
    ctx = solver._context(opts)
    ctx.set_reference(goals[:, :, None])
    ctx.set_model(ctx.model)
    r = ctx.sqp_solve_batch(x, u, N, DT, "PCG-SS")
    assert np.array_equal(r["x"], base["x"]) and np.array_equal(r["sqp_iter"], base["sqp_iter"])
    # R that is neither 1 nor B is an error that names both numbers
    from trajoptmpcreference_amd._native import NativeError
    ctx.set_reference(goals[:3, :, None])
    with pytest.raises(NativeError, match=r"R = 3.*\(4\)"):
        ctx.sqp_solve_batch(x, u, N, DT, "PCG-SS")
    ctx.set_reference(None)
