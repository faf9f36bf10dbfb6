"""Kernel-level parity of the tracking instances (per-knot goals from the goal window, tmpc_set_reference):
k_ilqr_backward / k_ilqr_forward through tmpc_ilqr_step_batch and the fused QP through tmpc_qp_batch, each with a
per-problem, per-knot reference.

iLQR: test_gpu_ilqr_kernels.py's comparisons and bounds.  K, d, dV against oracle/ilqr.py backward_hp (long double,
on the GPU's own A, B) with err_gpu <= 8 err_cpu64 + 1e-14, err_cpu64 the canonical-order CPU sweep, over a group
of 8 problems at one rho; every trial's rollout and cost against oilqr.forward / osqp.total_cost within that file's
FWD_BOUND["fp64"] (2.2e-11), trials with max|x| > 1e3 left out (at most a quarter).  The matrix-core sweep is
bitwise the VALU sweep (TMPC_ILQR_VALU=1), and the prefetching rollout bitwise the plain one (TMPC_ILQR_NOPF=1):
the goal rides the LDS-DMA prefetch in one and is read from the window in the other.

QP: one QP at one iterate against oracle/sqp.py solve_qp at test_gpu_sqp.py's tolerances for PCG-SS -- the QP's
PCG iteration count identical, values within 1e-7 relative (its rtol; test_gpu_pcg.py holds a single QP's dxul to
the same two bounds): arm6fix N = 66 (792 rows: the two-rows-per-lane register instance) and arm3
N = 8 on the HBM-row instance (TMPC_QP_GM_MIN_ROWS=1, as test_gpu_long_horizon.py sets it).
"""
import numpy as np
import pytest

import ilqr_cases as cases
from conftest import arm_model, quad_cost_arrays
from oracle import ilqr as oilqr
from oracle import sqp as osqp
from test_gpu_ilqr_kernels import FWD_BOUND, MARGIN64, SWEEP, TRIALS, _same
from tracking_cases import oracle_cost, reference

pytestmark = pytest.mark.gpu

B = 8
SHAPES = [("arm3", 2, 1e3), ("arm3", 8, 1e-3), ("arm6", 8, 1.0)]


@pytest.fixture(scope="module")
def kctx():
    from trajoptmpcreference_amd import _native
    c = _native.Context(0)
    yield c
    c.close()


def _step(ctx, key, N, rho, refs, trials=True):
    m = cases.model(key)
    x, u = cases.problems(key, N, B, 500)
    ctx.set_model(m)
    ctx.set_cost_quadratic(*quad_cost_arrays(m.n))
    ctx.set_options(precision=0, alpha_min_SQP_DDP=0.005, alpha_factor_SQP_DDP=0.5)
    ctx.set_box_limits(None)
    ctx.set_reference(refs)
    try:
        return ctx.ilqr_step_batch(x, u, N, cases.DT, np.full(B, rho), want_trials=trials)
    finally:
        ctx.set_reference(None)


def _refs(key, N):
    n = cases.model(key).n
    return np.array([reference(n, N, s) for s in range(B)])


@pytest.mark.parametrize("key,N,rho", SHAPES, ids=[f"{k}-N{N}" for k, N, _ in SHAPES])
def test_step_with_per_knot_reference_matches_oracle(kctx, key, N, rho):
    m = cases.model(key)
    x, u = cases.problems(key, N, B, 500)
    refs = _refs(key, N)
    r = _step(kctx, key, N, rho, refs)
    assert np.all(r["ok"] == 1)
    e_gpu = {"K": 0.0, "d": 0.0, "dV": 0.0}
    e_cpu = dict(e_gpu)
    T = len(r["alphas"])
    dev, left_out, total = 0.0, 0, 0
    for b in range(B):
        cost = oracle_cost(m.n, refs[b])
        dv = oilqr.derivatives(cost, x[b], u[b], N, None)
        ref = oilqr.backward_hp(r["A"][b], r["Bm"][b], *dv, rho)
        cpu = cases.cpu64_sweep(b, r["A"][b], r["Bm"][b], dv, rho)
        assert ref is not None and cpu is not None, b
        for e, got in ((e_gpu, (r["K"][b], r["d"][b], r["dV"][b, 0], r["dV"][b, 1])), (e_cpu, cpu)):
            e["K"] = max(e["K"], cases.rel_err(got[0], ref[0]))
            e["d"] = max(e["d"], cases.rel_err(got[1], ref[1]))
            e["dV"] = max(e["dV"], cases.rel_err([got[2], got[3]], [ref[2], ref[3]]))
        for t in range(T):
            total += 1
            with np.errstate(all="ignore"):
                xn, un = oilqr.forward(m, x[b], u[b], r["K"][b], r["d"][b], r["alphas"][t], cases.DT)
                Jn = osqp.total_cost(cost, xn, un, N, None)
            if not (np.all(np.isfinite(xn)) and np.all(np.isfinite(un)) and np.isfinite(Jn)):
                assert not (np.all(np.isfinite(r["xt"][b, t])) and np.isfinite(r["Jt"][b, t])), (b, t)
                left_out += 1
                continue
            if np.max(np.abs(xn)) > 1e3:
                left_out += 1
                continue
            e = max(cases.rel_err(r["xt"][b, t], xn), cases.rel_err(r["ut"][b, t], un),
                    cases.rel_err(r["Jt"][b, t], Jn))
            dev = max(dev, e)
            assert e <= FWD_BOUND["fp64"], (b, t, e)
    print(f"{key} N={N} rho={rho:g}: err_gpu {e_gpu} err_cpu64 {e_cpu}; forward deviation {dev:.3e}, "
          f"{left_out} of {total} trials left out")
    for what in e_gpu:
        assert e_gpu[what] <= MARGIN64 * e_cpu[what] + 1e-14, (what, e_gpu[what], e_cpu[what])
    assert 4 * left_out <= total, (left_out, total)
    # the reference is used at all: the fixed-goal sweep of the same problems differs
    kctx.set_reference(None)
    fixed = kctx.ilqr_step_batch(x, u, N, cases.DT, np.full(B, rho), want_trials=False)
    assert not np.array_equal(fixed["d"], r["d"])


@pytest.mark.parametrize("key,N,rho", SHAPES, ids=[f"{k}-N{N}" for k, N, _ in SHAPES])
def test_tracking_matrix_core_sweep_and_prefetch_are_bitwise_their_plain_forms(kctx, key, N, rho, monkeypatch):
    refs = _refs(key, N)
    a = _step(kctx, key, N, rho, refs)
    monkeypatch.setenv("TMPC_ILQR_VALU", "1")
    b = _step(kctx, key, N, rho, refs)
    monkeypatch.delenv("TMPC_ILQR_VALU")
    for f in SWEEP + TRIALS:
        assert _same(a[f], b[f]), ("VALU", f)
    monkeypatch.setenv("TMPC_ILQR_NOPF", "1")
    c = _step(kctx, key, N, rho, refs)
    for f in SWEEP + TRIALS:
        assert _same(a[f], c[f]), ("NOPF", f)


def _rel(a, b):
    return float(np.max(np.abs(np.asarray(a) - np.asarray(b)))) / max(1.0, float(np.max(np.abs(b))))


@pytest.mark.parametrize("name,N,gm", [("arm6fix", 66, False), ("arm3", 8, True)],
                         ids=["arm6fix-N66-two-rows-per-lane", "arm3-N8-hbm-rows"])
def test_qp_with_per_knot_reference_matches_oracle(kctx, name, N, gm, monkeypatch):
    if gm:
        monkeypatch.setenv("TMPC_QP_GM_MIN_ROWS", "1")
    m = arm_model(name)
    xref = reference(m.n, N, 0)
    x, u = osqp.initial_problem(m, N, 0.1, 3)
    u = np.random.default_rng(3).uniform(-0.2, 0.2, u.shape)   # an iterate with defects and controls
    rho = 1e-3
    kctx.set_model(m)
    kctx.set_cost_quadratic(*quad_cost_arrays(m.n))
    kctx.set_options(precision=0)
    kctx.set_box_limits(None)
    kctx.set_reference(xref[None])
    try:
        r = kctx.qp_batch(x[None], u[None], N, 0.1, rho, "PCG-SS", want_blocks=False)
    finally:
        kctx.set_reference(None)
    o = osqp.default_options({})
    dxul, iters, _ = osqp.solve_qp(m, oracle_cost(m.n, xref), x, u, x[:, 0].copy(), N, 0.1, rho, "PCG-SS", o)
    print(f"{name} N={N}: pcg iters gpu {int(r['pcg_iters'][0])} oracle {iters}, "
          f"dxul rel err {_rel(r['dxul'][0], np.ravel(dxul)):.3e}")
    assert int(r["pcg_iters"][0]) == iters
    assert _rel(r["dxul"][0], np.ravel(dxul)) < 1e-7
    fixed = kctx.qp_batch(x[None], u[None], N, 0.1, rho, "PCG-SS", want_blocks=False)
    assert not np.array_equal(fixed["dxul"], r["dxul"])
