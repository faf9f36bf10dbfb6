"""GPU: the plant step is one rule (the integrator section of csrc/tmpc_device.h).

Every kernel that advances a state evaluates state_qdd's lines and euler_next of that section, so on the same
(x, u, dt) they give the same bits.  With f = fd_batch(x, u, dt)[0] (k_unit_fd) on K = 65 knots of dyn_cases'
states (a partial workgroup), no tolerance anywhere:
  * k_rollout: state 1 of rollout_device with N = 2, B = 65 (two 64-lane workgroups, the second partial);
  * k_mpc_advance: x_pred of one mpc_step (step 0, N = 4, B = 3, iLQR, which leaves x_0 as given) is fd_batch of
    the solve's own (x_0, u_0);
  * k_qp_fd: c[:, k + 1] of qp_last_inputs after a qp_batch whose trajectory has x[:, :, k + 1] = 0 is
    0.0 - f(x_k, u_k) (a subtraction, so a zero keeps its sign); one qp_batch per k, since knot k + 1 is knot k
    of the next defect;
  * euler_jac_store: the first NJ rows of fd_grad_batch's A are exactly 1, dt and 0 and those of B are +0, the
    structure k_qp builds its rows on.
k_ls_terms and k_ilqr_forward expose no single step through the ABI: what holds them is the existing parity tests
(test_gpu_sqp.py, test_gpu_ilqr_kernels.py, test_gpu_tracking_kernels.py) and the byte comparison of every site's
outputs between the library before and after the section was written (profiles/euler_step/README.md).
"""
import numpy as np
import pytest

import dyn_cases as dc
from conftest import quad_cost_arrays

pytestmark = pytest.mark.gpu

MODELS = ["arm1", "arm3", "arm6", "tree7"]   # tree7: two joints on the base, two branch points, two prismatic
K = 65


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _same(a, b):
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


@pytest.fixture(scope="module")
def ectx():
    from trajoptmpcreference_amd import _native
    c = _native.Context(0)
    yield c
    c.close()


_step = {}


def _load(ctx, key, monkeypatch):
    """the model as set_model dispatches it, fp64, with a cost for the solver-side calls; returns (x, u, f)"""
    monkeypatch.setenv("TMPC_GENERIC_MODEL", "0")
    m = dc.model(key)
    ctx.set_model(m)
    ctx.set_options(precision=0, pcg_warm_start=0, max_iter_SQP_DDP=2)
    ctx.set_box_limits(None)
    ctx.set_reference(None)
    ctx.set_cost_quadratic(*quad_cost_arrays(m.n))
    x, u = dc.states(key, K)
    if key not in _step:
        f = ctx.fd_batch(x, u, dc.DT, want_minv=False)[0]
        f.setflags(write=False)
        _step[key] = f
    return x, u, _step[key]


@pytest.mark.parametrize("key", MODELS)
def test_rollout_is_the_unit_step(ectx, key, monkeypatch):
    x, u, f = _load(ectx, key, monkeypatch)
    nx, N = x.shape[1], 2
    xd = np.zeros((K, nx, N))
    xd[:, :, 0] = x
    ud = np.ascontiguousarray(u[:, :, None])   # [B][nu][N - 1]
    d_x, d_u = ectx.alloc(xd.nbytes), ectx.alloc(ud.nbytes)
    try:
        ectx.h2d(d_x, xd)
        ectx.h2d(d_u, ud)
        ectx.rollout_device(K, N, dc.DT, d_x, d_u)
        ectx.d2h(xd, d_x)
    finally:
        ectx.free(d_x)
        ectx.free(d_u)
    assert _same(xd[:, :, 0], x)
    assert _same(xd[:, :, 1], f)


@pytest.mark.parametrize("key", MODELS)
def test_mpc_step_prediction_is_the_unit_step(ectx, key, monkeypatch):
    x, u, _ = _load(ectx, key, monkeypatch)
    n, nx, N, B = u.shape[1], x.shape[1], 4, 3
    xt = np.ascontiguousarray(x[:B * N].reshape(B, N, nx).transpose(0, 2, 1))
    ut = np.ascontiguousarray(u[:B * N].reshape(B, N, n)[:, :N - 1].transpose(0, 2, 1))
    r = ectx.mpc_step(xt, ut, N, dc.DT, "iLQR", 0)
    assert np.all(np.isfinite(r["u0"]))
    want = ectx.fd_batch(xt[:, :, 0], r["u0"], dc.DT, want_minv=False)[0]
    assert _same(r["x_pred"], want)
    assert _same(r["x"][:, :, 0], want)   # the shifted horizon starts at the prediction


@pytest.mark.parametrize("key", MODELS)
def test_qp_defect_is_the_unit_step(ectx, key, monkeypatch):
    x, u, f = _load(ectx, key, monkeypatch)
    n, nx, N, B = u.shape[1], x.shape[1], 4, 3
    xt = np.ascontiguousarray(x[:B * N].reshape(B, N, nx).transpose(0, 2, 1))
    ut = np.ascontiguousarray(u[:B * N].reshape(B, N, n)[:, :N - 1].transpose(0, 2, 1))
    fk = f[:B * N].reshape(B, N, nx)
    c = np.full((B, N - 1, nx), np.nan)
    for k in range(N - 1):
        xz = xt.copy()
        xz[:, :, k + 1] = 0.0
        ectx.qp_batch(xz, ut, N, dc.DT, 1.0, "PCG-SS", want_blocks=False)
        c[:, k] = ectx.qp_last_inputs(B, N)["c"][:, k + 1]
    assert _same(c, 0.0 - fk[:, :N - 1])


@pytest.mark.parametrize("key", ["arm3", "tree7"])
def test_jacobian_top_rows_are_structural(ectx, key, monkeypatch):
    x, u, _ = _load(ectx, key, monkeypatch)
    n = u.shape[1]
    A, Bm, _ = ectx.fd_grad_batch(x, u, dc.DT)
    top = np.hstack([np.eye(n), dc.DT * np.eye(n)])
    assert np.array_equal(A[:, :n], np.broadcast_to(top, (K, n, 2 * n)))
    assert _same(Bm[:, :n], np.zeros((K, n, n)))   # +0, not -0
    assert np.any(A[:, n:] != 0.0) and np.any(Bm[:, n:] != 0.0)
