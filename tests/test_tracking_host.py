"""Per-problem goals and per-knot references, the parts that need no GPU: TrackingCost's host hooks against the
oracle-side TrackCost, its routing to the device path, the argument errors of goal= (raised before any device
work) and the two entry points on a null context."""
import numpy as np
import pytest

from conftest import quad_cost_arrays
from tracking_cases import TrackCost, fixed_solver, plant, reference, tracking_solver


@pytest.mark.parametrize("M", [1, 5, 8, 11])
def test_tracking_cost_hooks_match_the_oracle_side(M):
    from trajoptmpcreference_amd import TrackingCost
    n, N = 3, 8
    Q, QF, R, _ = quad_cost_arrays(n)
    xref = reference(n, M, 2)
    ours, ref = TrackingCost(Q, QF, R, xref), TrackCost(Q, QF, R, xref)
    rng = np.random.default_rng(0)
    for step in range(4):
        ref.step = step
        assert ours.shift == step
        for k in range(N):
            x, u = rng.standard_normal(2 * n), rng.standard_normal(n)
            uk = None if k == N - 1 else u
            assert ours.value(x, uk, k) == ref.value(x, uk, k)
            assert np.array_equal(ours.gradient(x, uk, k), ref.gradient(x, uk, k))
            assert np.array_equal(ours.goal(k), xref[:, min(k + step, M - 1)])
            assert np.array_equal(ours.hessian(x, uk, k), ref.hessian(uk is None, k))
        assert np.array_equal(ours.window()[:, 0], xref[:, min(step, M - 1)])
        assert ours.shift_reference() == step + 1
    assert ours.shift_reference(3) == 7


def test_tracking_cost_rejects_bad_references():
    from trajoptmpcreference_amd import TrackingCost
    Q, QF, R, _ = quad_cost_arrays(3)
    with pytest.raises(ValueError):
        TrackingCost(Q, QF, R, np.zeros((5, 4)))        # nx = 6 rows expected
    with pytest.raises(ValueError):
        TrackingCost(Q, QF, R, np.zeros((6, 0)))
    assert TrackingCost(Q, QF, R, np.ones(6)).xref.shape == (6, 1)   # a vector: a constant goal


def test_tracking_cost_is_a_device_cost():
    from trajoptmpcreference_amd import TrackingCost, hooks
    s = tracking_solver("arm3", reference(3, 8, 0))
    assert hooks.device_cost(s.cost) is s.cost
    assert not hooks.needs_hooks(s.plant, s.cost, s.other_constraints)

    class Mine(TrackingCost):   # a caller's own hook still takes the plugin-hook path
        def value(self, *a, **k):
            return 0.0
    Q, QF, R, _ = quad_cost_arrays(3)
    assert hooks.device_cost(Mine(Q, QF, R, reference(3, 8, 0))) is None


@pytest.mark.parametrize("entry", ["SQP_batch", "iLQR_batch", "MPC_batch"])
def test_goal_argument_errors_come_before_any_device_work(entry, monkeypatch):
    s = fixed_solver("arm3")
    # any device work would go through the plant's context: make that an error of its own kind
    monkeypatch.setattr(type(s.plant), "_ctx", lambda self: (_ for _ in ()).throw(AssertionError("device touched")))
    B, N, nx = 4, 8, 6
    x, u = np.zeros((B, nx, N)), np.zeros((B, 3, N - 1))
    call = getattr(s, entry)
    for bad in (np.zeros((B, nx + 1)), np.zeros((B, nx, 0)), np.zeros(nx), np.zeros((B, 2, nx, 3))):
        with pytest.raises(ValueError, match="goal must be"):
            call(x, u, N, 0.1, goal=bad)
    for R in (2, 3, 5):
        with pytest.raises(ValueError, match=f"R = {R} rows: must be 1 or the batch size B \\({B}\\)"):
            call(x, u, N, 0.1, goal=np.zeros((R, nx, N)))


def test_goal_with_urdf_cost_is_refused_before_any_device_work(monkeypatch):
    from trajoptmpcreference_amd import TrajoptMPCReference, UrdfCost
    p = plant("arm2")
    s = TrajoptMPCReference(p, UrdfCost(p, np.eye(4), np.eye(4), np.eye(2), np.zeros(4)))
    monkeypatch.setattr(type(p), "_ctx", lambda self: (_ for _ in ()).throw(AssertionError("device touched")))
    with pytest.raises(NotImplementedError, match="UrdfCost"):
        s.SQP_batch(np.zeros((2, 4, 4)), np.zeros((2, 2, 3)), 4, 0.1, goal=np.zeros((2, 4)))


def test_stream_goal_shape_errors_need_no_device():
    from trajoptmpcreference_amd import _native
    with pytest.raises(ValueError, match="stream's period \\(6\\)"):
        _native.reference_array(np.zeros((4, 6, 8)), 6, 6, "stream's period")
    assert _native.reference_array(np.zeros((6, 6)), 6, 6).shape == (6, 6, 1)
    assert _native.reference_array(np.zeros((1, 6, 9)), 6, 6).shape == (1, 6, 9)


def test_reference_entry_points_refuse_a_null_context():
    from trajoptmpcreference_amd import _native
    lib = _native.load_library()
    a = np.zeros(12)
    assert lib.tmpc_set_reference(None, 1, 2, a.ctypes.data_as(_native._dp)) < 0
    assert lib.tmpc_set_reference_device(None, 1, 2, None) < 0
    assert lib.tmpc_set_reference(None, 0, 0, None) < 0
