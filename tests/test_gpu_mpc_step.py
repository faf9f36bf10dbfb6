"""GPU: the closed-loop MPC step (tmpc_mpc_step_device, MPCSession).

One call is one iteration of oracle/mpc.py's loop with a measured state injected at its top, so
  * stepping with no measurement, or with the previous step's x_pred as the measurement, is MPC_batch bit for bit
    (np.array_equal on everything the loop returns).  Both run the same step (mpc_one_step, k_mpc_advance), so
    this holds the Python mirrors, the x_meas copy, the output addressing of the two callers and the rules of a
    continued loop;
  * the shift itself -- x, u and the soft constants across each 64-knot chunk edge of k_mpc_advance -- is the
    loop restated in NumPy around SQP_batch, again bit for bit;
  * a disturbed measurement steers the solve as it steers the oracle's loop (integers identical, values within
    the existing MPC tests' rtol 1e-6 / atol 1e-8);
  * a step that does not continue the context's previous one is refused with what was expected.
"""
import numpy as np
import pytest

from conftest import arm_model, quad_cost_arrays
from test_gpu_mpc import _setup
from tracking_cases import reference, tracking_solver

pytestmark = pytest.mark.gpu

DT = 0.1
TORQUE_AL = {"torque": ([-0.7] * 3, [0.7] * 3, "AUGMENTED_LAGRANGIAN")}


def _problems(name, N, B, seed0):
    from oracle import sqp as osqp
    m = arm_model(name)
    xs, us = zip(*[osqp.initial_problem(m, N, DT, seed0 + i) for i in range(B)])
    return np.array(xs), np.array(us)


def _run_session(solver, x, u, N, method, opts, steps, measure=None, goal=None):
    """`steps` steps of a session; measure(s, previous step's result) -> x_meas of step s >= 1 (None: none)"""
    outs = []
    with solver.MPC_session(x, u, N, DT, method, dict(opts), goal=goal) as s:
        for k in range(steps):
            xm = measure(k, outs[-1]) if (measure and k) else None
            outs.append(s.step(xm))
        hx, hu = s.horizon()
        soft = s.soft_state()
    return outs, hx, hu, soft


def _assert_is_the_loop(outs, hx, hu, soft, r):
    for s, o in enumerate(outs):
        assert np.array_equal(o["u0"], r["u_exec"][:, :, s]), s
        assert np.array_equal(o["x_pred"], r["x_exec"][:, :, s + 1]), s
        assert np.array_equal(o["exit_code"], r["exit_codes"][:, s]), s
        assert np.array_equal(o["iters"], r["iters"][:, s]), s
    assert np.array_equal(hx, r["x"]) and np.array_equal(hu, r["u"])
    if "soft_state" in r:
        for a, b in zip(soft, r["soft_state"]):
            assert np.array_equal(a, b)
    else:
        assert soft is None


LOOP_CASES = [(m, v) for v in ("plain", "torque_al", "goal") for m in ("iLQR", "QP-PCG-SS", "QP-S")] + \
             [("QP-PCG-SS", "warm")]


@pytest.mark.parametrize("method,variant", LOOP_CASES)
def test_steps_equal_the_loop(method, variant):
    """test_gpu_mpc.py's shapes; x_meas = None and x_meas = the previous x_pred both give MPC_batch's bits"""
    N, B, steps = 16, 4, 3
    x, u = _problems("arm3", N, B, 700)
    opts = {"max_iter_SQP_DDP": 8}
    goal = None
    if variant == "warm":
        opts["pcg_warm_start"] = True
    if variant == "goal":
        goal = np.array([reference(3, N + 2, i) for i in range(B)])   # [B][nx][N + 2]: the window slides

    def solver():
        return _setup(3, N, QF_start=12, spec=TORQUE_AL if variant == "torque_al" else None)
    s0 = solver()
    r = s0.MPC_batch(x, u, N, DT, method, dict(opts), mpc_steps=steps, goal=goal)
    assert s0.cost.QF_start == 12 - steps
    for measure in (None, lambda k, prev: prev["x_pred"]):
        s1 = solver()
        _assert_is_the_loop(*_run_session(s1, x, u, N, method, opts, steps, measure, goal), r)
        assert s1.cost.QF_start == 12 - steps


def _numpy_loop(solver, x, u, N, opts, x_exec, steps):
    """oracle/mpc.py's loop around SQP_batch with the shifts in NumPy: without pcg_warm_start, step s of MPC_batch
    is SQP_batch's solve of the current horizon and soft state.  The plant is not restated: the state after step
    s is x_exec[:, :, s + 1] of the loop under test (test_gpu_mpc.py holds it against the oracle's).  The soft
    constants shift as BoxConstraint.shift_soft_constraint_constants(1) does: knot 0 takes knot 1, every later
    knot of a slot's span returns to (mu_init, 0, phi_init) of the slot's kind; the torque slots (the last 2 n of
    6 n) span N - 1 knots.  A kind without limits has no constants: its tmpc_box_limits row stays zero
    (Context.set_box_limits), and its slots, which no solve reads, return to zero."""
    n = u.shape[1]
    con = solver.other_constraints
    init = np.zeros((3, 6 * n))   # (mu, lam, phi) per slot
    for t, kind in enumerate(con.KINDS):
        c = getattr(con, kind)
        if c is not None:
            init[0, 2 * n * t:2 * n * (t + 1)] = c.options["quadratic_penalty_mu_init"]
            init[2, 2 * n * t:2 * n * (t + 1)] = c.options["augmentated_lagrangian_phi_init"]
    span = np.array([N] * 4 * n + [N - 1] * 2 * n)
    x, u, soft = x.copy(), u.copy(), None
    u_exec, codes, iters = [], [], []
    for s in range(steps):
        r = solver.SQP_batch(x, u, N, DT, "PCG-SS", dict(opts), soft_state=soft)
        x, u, soft = r["x"].copy(), r["u"].copy(), [a.copy() for a in r["soft_state"]]
        u_exec.append(u[:, :, 0].copy())
        codes.append(r["exit_sqp"])
        iters.append(r["sqp_iter"])
        x[..., :-1] = x[..., 1:].copy()
        x[..., 0] = x_exec[:, :, s + 1]
        u[..., :-1] = u[..., 1:].copy()
        for a, a0 in zip(soft, init):
            a[:, 0] = a[:, 1]
            for k in range(1, N):
                a[:, k, k < span] = a0[k < span]
    return dict(x=x, u=u, soft_state=soft, u_exec=np.stack(u_exec, axis=2), exit_codes=np.stack(codes, axis=1),
                iters=np.stack(iters, axis=1))


@pytest.mark.parametrize("N", [3, 64, 65, 66, 129, 130])
def test_chunked_shift_across_the_chunk_edges(N):
    """k_mpc_advance shifts 64 knots per chunk: one knot either side of each chunk edge (N - 1 = 63 .. 65 and
    128, 129 shifted knots) and the smallest horizon, with every array the kernel moves in play -- x, u, the warm
    lambda, the soft constants (torque rows: N - 1 knots).  arm2 at N = 130 is 520 Schur rows: the fused QP.
    Two statements: the session's steps are the loop's with the warm lambda in play (the output addressing of both
    callers), and, with a cold PCG, the loop is SQP_batch with the shifts restated in NumPy (the shift itself;
    the warm lambda has no accessor and is not part of this one)."""
    B, steps = 2, 2
    x, u = _problems("arm2", N, B, 740)
    opts = {"max_iter_SQP_DDP": 2, "max_iter_softConstraints": 2, "pcg_warm_start": True}
    spec = {"torque": ([-0.7] * 2, [0.7] * 2, "AUGMENTED_LAGRANGIAN")}
    r = _setup(2, N, spec=spec).MPC_batch(x, u, N, DT, "QP-PCG-SS", dict(opts), mpc_steps=steps)
    _assert_is_the_loop(*_run_session(_setup(2, N, spec=spec), x, u, N, "QP-PCG-SS", opts, steps), r)

    cold = {k: v for k, v in opts.items() if k != "pcg_warm_start"}
    r = _setup(2, N, spec=spec).MPC_batch(x, u, N, DT, "QP-PCG-SS", dict(cold), mpc_steps=steps)
    assert np.array_equal(r["x_exec"][:, :, 0], x[:, :, 0])
    e = _numpy_loop(_setup(2, N, spec=spec), x, u, N, cold, r["x_exec"], steps)
    for key in ("u_exec", "exit_codes", "iters", "x", "u"):
        assert np.array_equal(r[key], e[key]), key
    for a, b in zip(r["soft_state"], e["soft_state"]):
        assert np.array_equal(a, b)


# ---------------------------------------------------------------------------------------------- measurements
def disturbances(B, nx, steps):
    """d [B][steps - 1][nx]: problem i's disturbance of steps 1 .. steps - 1, uniform +-0.05 from
    default_rng(900 + i)"""
    return np.array([np.random.default_rng(900 + i).uniform(-0.05, 0.05, (steps - 1, nx)) for i in range(B)])


def oracle_measured_loop(m, cost, x, u, N, method, steps, opts, d, soft=None, warm=False, jitter=None):
    """oracle/mpc.py's body with x[:, 0] = x_meas at the top: x_meas = the previous step's x_pred + d[s - 1]
    (times 1 + jitter[s - 1], the CPU stability check of the integers) at steps s >= 1.  Returns per step
    (u0, x_pred, exit code, iterations)."""
    from oracle import ilqr as oilqr
    from oracle import mpc as ompc
    from oracle import rbd
    from oracle import sqp as osqp
    x, u = np.array(x, dtype=float), np.array(u, dtype=float)
    nx = x.shape[0]
    wd = {"lam": None} if warm and method.startswith("PCG") else None
    out, x_pred = [], None
    for s in range(steps):
        if s:
            xm = x_pred + d[s - 1]
            x[:, 0] = xm if jitter is None else xm * (1.0 + jitter[s - 1])
        if method == "iLQR":
            r = oilqr.ilqr(m, cost, x, u, N, DT, dict(opts), soft)
            code, it = r["exit_code"], r["iter"]
        else:
            r = osqp.sqp(m, cost, x, u, N, DT, method, dict(opts), soft, wd)
            code, it = r["exit_sqp"], r["sqp_iter"]
        x, u = r["x"], r["u"]
        x_pred = rbd.euler(m, x[:, 0][None], u[:, 0][None], DT)[0]
        out.append((u[:, 0].copy(), x_pred.copy(), int(code), int(it)))
        x = np.concatenate([x[:, 1:], x[:, -1:]], axis=1)
        u = np.concatenate([u[:, 1:], u[:, -1:]], axis=1)
        x[:, 0] = x_pred
        if cost.QF_start is not None:
            cost.QF_start = max(cost.QF_start - 1, 0)
        ompc.shift_soft(soft)
        if wd is not None and wd["lam"] is not None:
            L = wd["lam"].reshape(N, nx)
            wd["lam"] = np.concatenate([L[1:], L[-1:]]).reshape(-1)
    return out


# (GPU method, options, soft limits): the three solvers, and QP-S under AL torque limits
MEASURED = {
    "iLQR": ("iLQR", {"max_iter_SQP_DDP": 8}, False),
    "QP-PCG-SS-warm": ("QP-PCG-SS", {"max_iter_SQP_DDP": 8, "pcg_warm_start": True}, False),
    "QP-S": ("QP-S", {"max_iter_SQP_DDP": 8}, False),
    "QP-S-torque-al": ("QP-S", {"max_iter_SQP_DDP": 6, "max_iter_softConstraints": 3}, True),
}
MEASURED_SHAPE = dict(N=16, B=4, steps=4, seed0=800, QF_start=12)


def oracle_measured_case(case, i, x, u, jitter=None):
    """problem i of MEASURED[case] through the oracle's measured loop"""
    from oracle import sqp as osqp
    from oracle.soft import SoftConstraints, SoftLimit
    method, opts, al = MEASURED[case]
    sh = MEASURED_SHAPE
    N, steps = sh["N"], sh["steps"]
    soft = SoftConstraints([SoftLimit("torque", 3, N, [-0.7] * 3, [0.7] * 3, "AUGMENTED_LAGRANGIAN")]) if al else None
    cost = osqp.QuadCost(*quad_cost_arrays(3), QF_start=sh["QF_start"])
    oopts = {k: v for k, v in opts.items() if k != "pcg_warm_start"}
    return oracle_measured_loop(arm_model("arm3"), cost, x[i], u[i], N, "iLQR" if method == "iLQR" else method[3:],
                                steps, oopts, disturbances(sh["B"], 6, steps)[i], soft,
                                warm=bool(opts.get("pcg_warm_start")), jitter=jitter)


@pytest.mark.parametrize("case", list(MEASURED))
def test_measurements_steer_the_solve(case):
    """Steps 1..3 restart from x_pred + d: per step the exit codes and iteration counts are the oracle loop's,
    u0 and x_pred within the MPC tests' bound, and over steps 1..3 u0 leaves the nominal run's by more than that
    bound (an ignored measurement fails; on the CPU oracle the largest difference per run is at least 9e-3 -- a
    single step may show none: an SQP solve that accepts no step returns its warm start's u0).  Each side disturbs its own x_pred, so the two measurements differ by the
    parity error (~1e-12 relative); the integers of all 16 (case, problem) runs, the AL torque case's seeds
    included, were checked on the CPU to stay put under a +-1e-12 relative jitter of every measurement (this
    module's oracle_measured_case with jitter=, five draws per run), so they are stable against it."""
    method, opts, al = MEASURED[case]
    sh = MEASURED_SHAPE
    N, B, steps = sh["N"], sh["B"], sh["steps"]
    x, u = _problems("arm3", N, B, sh["seed0"])
    d = disturbances(B, 6, steps)

    def solver():
        return _setup(3, N, QF_start=sh["QF_start"], spec=TORQUE_AL if al else None)
    outs, _, _, _ = _run_session(solver(), x, u, N, method, opts, steps, lambda k, prev: prev["x_pred"] + d[:, k - 1])
    nominal = solver().MPC_batch(x, u, N, DT, method, dict(opts), mpc_steps=steps)
    for i in range(B):
        o = oracle_measured_case(case, i, x, u)
        for s in range(steps):
            u0, xp, code, it = o[s]
            print(case, i, s, int(outs[s]["exit_code"][i]), code, int(outs[s]["iters"][i]), it,
                  float(np.max(np.abs(outs[s]["u0"][i] - u0))), float(np.max(np.abs(outs[s]["x_pred"][i] - xp))))
            assert int(outs[s]["exit_code"][i]) == code, (i, s)
            assert int(outs[s]["iters"][i]) == it, (i, s)
            assert np.allclose(outs[s]["u0"][i], u0, rtol=1e-6, atol=1e-8), (i, s)
            assert np.allclose(outs[s]["x_pred"][i], xp, rtol=1e-6, atol=1e-8), (i, s)
        assert np.array_equal(outs[0]["u0"][i], nominal["u_exec"][i, :, 0])   # step 0 has no measurement
        steered = np.array([outs[s]["u0"][i] for s in range(1, steps)]).T
        assert not np.allclose(steered, nominal["u_exec"][i, :, 1:], rtol=1e-6, atol=1e-8), i


# ---------------------------------------------------------------------------------------------- refusals
def _own_context(solver, **opts):
    o = dict(opts)
    solver.set_default_options(o)
    return solver._context(o, own=True)


def test_a_step_that_does_not_continue_the_loop_is_refused():
    from trajoptmpcreference_amd import _native
    N, B = 8, 4
    x, u = _problems("arm3", N, B, 760)
    solver = _setup(3, N)
    ctx = _own_context(solver, max_iter_SQP_DDP=2, pcg_warm_start=True)
    try:
        with pytest.raises(_native.NativeError, match="MPC step 1: the context's previous solve was not an MPC step"):
            ctx.mpc_step(x, u, N, DT, "PCG-SS", 1)                       # a fresh context
        r0 = ctx.mpc_step(x, u, N, DT, "PCG-SS", 0)
        with pytest.raises(_native.NativeError, match="previous solve was step 0 of B=4, N=8.*expected step 1"):
            ctx.mpc_step(r0["x"], r0["u"], N, DT, "PCG-SS", 2)           # a skipped step
        with pytest.raises(_native.NativeError, match="previous solve was step 0 of B=4, N=8.*expected step 1"):
            ctx.mpc_step(r0["x"][:3], r0["u"][:3], N, DT, "PCG-SS", 1)   # a changed batch
        with pytest.raises(_native.NativeError, match="solver=1.*previous solve was step 0.*solver=4"):
            ctx.mpc_step(r0["x"], r0["u"], N, DT, "S", 1)                # a changed solver
        r1 = ctx.mpc_step(r0["x"], r0["u"], N, DT, "PCG-SS", 1)          # a refusal leaves the loop as it was
        ctx.sqp_solve_batch(x, u, N, DT, "PCG-SS", with_trace=False)
        with pytest.raises(_native.NativeError, match="MPC step 2: the context's previous solve was not an MPC step"):
            ctx.mpc_step(r1["x"], r1["u"], N, DT, "PCG-SS", 2)           # another solve in between
        with pytest.raises(_native.NativeError, match="step must be >= 0"):
            ctx.mpc_step(x, u, N, DT, "PCG-SS", -1)
        # a solver id that is neither a TMPC_LINSYS_* nor TMPC_SOLVER_ILQR
        assert ctx.lib.tmpc_mpc_step_device(ctx.h, B, N, DT, 9, 0, None, None, None) < 0
        assert b"use TMPC_LINSYS" in ctx.lib.tmpc_last_error(ctx.h)
    finally:
        ctx.close()
    # the two accepted steps were the loop's
    ref = _setup(3, N).MPC_batch(x, u, N, DT, "QP-PCG-SS", {"max_iter_SQP_DDP": 2, "pcg_warm_start": True}, mpc_steps=2)
    assert np.array_equal(r1["x"], ref["x"]) and np.array_equal(r1["u0"], ref["u_exec"][:, :, 1])


def test_the_loops_refusals_are_the_steps():
    from trajoptmpcreference_amd import (QuadraticCost, TrajoptMPCReference, URDFPlant, UrdfCost, _native,
                                         planar_arm_urdf)
    N = 8
    wide = TrajoptMPCReference(URDFPlant(options={"path_to_urdf": planar_arm_urdf(9)}),
                               QuadraticCost(*quad_cost_arrays(9)))
    ctx = _own_context(wide)
    try:
        with pytest.raises(_native.NativeError, match="MPC loop supports up to 7 joints"):
            ctx.mpc_step(np.zeros((1, 18, N)), np.zeros((1, 9, N - 1)), N, DT, "PCG-SS", 0)
    finally:
        ctx.close()
    p = URDFPlant(options={"path_to_urdf": planar_arm_urdf(2)})
    ee = TrajoptMPCReference(p, UrdfCost(p, np.eye(4), np.eye(4), np.eye(2), np.zeros(4)))
    ctx = _own_context(ee)
    try:
        with pytest.raises(_native.NativeError, match="MPC loop supports QuadraticCost only"):
            ctx.mpc_step(np.zeros((1, 4, N)), np.zeros((1, 2, N - 1)), N, DT, "PCG-SS", 0)
    finally:
        ctx.close()
    with pytest.raises(NotImplementedError, match="QuadraticCost only"):
        ee.MPC_session(np.zeros((1, 4, N)), np.zeros((1, 2, N - 1)), N, DT)


# ---------------------------------------------------------------------------------------------- the session
def test_session_is_undisturbed_by_other_solves_on_its_solver():
    N, B, steps = 16, 4, 3
    x, u = _problems("arm3", N, B, 700)
    opts = {"max_iter_SQP_DDP": 8, "pcg_warm_start": True}
    plain = _run_session(_setup(3, N, QF_start=12, spec=TORQUE_AL), x, u, N, "QP-PCG-SS", opts, steps)
    solver = _setup(3, N, QF_start=12, spec=TORQUE_AL)
    outs = []
    with solver.MPC_session(x, u, N, DT, "QP-PCG-SS", dict(opts)) as s:
        for k in range(steps):
            if k == 2:   # the plant's shared context: another batch, other options, its own soft state
                solver.SQP_batch(x[:2], u[:2], N, DT, "PCG-SS", {"max_iter_SQP_DDP": 3})
            outs.append(s.step())
            assert solver.cost.QF_start == 12 - (k + 1) and s.steps_done == k + 1
        hx, hu = s.horizon()
        soft = s.soft_state()
    for a, b in zip(outs, plain[0]):
        for key in ("u0", "x_pred", "exit_code", "iters"):
            assert np.array_equal(a[key], b[key]), key
    assert np.array_equal(hx, plain[1]) and np.array_equal(hu, plain[2])
    for a, b in zip(soft, plain[3]):
        assert np.array_equal(a, b)
    hx2, _ = s.horizon()   # closed: the last horizon stays readable
    assert np.array_equal(hx2, hx)


def test_session_moves_a_tracking_costs_shift_with_the_loop():
    N, B, steps = 16, 4, 3
    x, u = _problems("arm3", N, B, 700)
    xref = reference(3, N + 2, 0)
    opts = {"max_iter_SQP_DDP": 8}
    r = tracking_solver("arm3", xref).MPC_batch(x, u, N, DT, "QP-PCG-SS", dict(opts), mpc_steps=steps)
    solver = tracking_solver("arm3", xref)
    outs = []
    with solver.MPC_session(x, u, N, DT, "QP-PCG-SS", dict(opts)) as s:
        for k in range(steps):
            outs.append(s.step())
            assert solver.cost.shift == k + 1
        hx, hu = s.horizon()
    _assert_is_the_loop(outs, hx, hu, None, r)
    # goal= replaces the cost's reference for the session: its shift stays
    with solver.MPC_session(x, u, N, DT, "QP-PCG-SS", dict(opts), goal=xref[None]) as s:
        s.step()
    assert solver.cost.shift == steps
