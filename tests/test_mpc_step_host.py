"""The closed-loop MPC step (tmpc_mpc_step / tmpc_mpc_step_device, MPCSession), the parts that need no GPU: the
entry points on a null context, the layout of tmpc_mpc_io and the argument errors of an MPCSession, which are
raised before any device work."""
import ctypes

import numpy as np
import pytest

from tracking_cases import fixed_solver, plant


def test_step_entry_points_refuse_a_null_context():
    from trajoptmpcreference_amd import _native
    lib = _native.load_library()
    io = _native.tmpc_mpc_io()
    assert lib.tmpc_mpc_step_device(None, 1, 4, 0.1, 4, 0, None, None, ctypes.byref(io)) < 0
    assert lib.tmpc_mpc_step_device(None, 1, 4, 0.1, 4, 0, None, None, None) < 0
    assert lib.tmpc_mpc_step(None, 1, 4, 0.1, 4, 0, None, None, ctypes.byref(io)) < 0
    assert lib.tmpc_mpc_step(None, 1, 4, 0.1, 16, 3, None, None, None) < 0


def test_mpc_io_struct_layout():
    """tmpc_mpc_io: four pointers in the header's order"""
    from trajoptmpcreference_amd import _native
    assert [f[0] for f in _native.tmpc_mpc_io._fields_] == ["x_meas", "u0", "x_pred", "status"]
    assert ctypes.sizeof(_native.tmpc_mpc_io) == 32
    assert all(ctypes.sizeof(f[1]) == 8 for f in _native.tmpc_mpc_io._fields_)


def _no_device(monkeypatch):
    """any device work goes through a context: make creating or fetching one an error of its own kind"""
    from trajoptmpcreference_amd import _native

    def touched(*a, **k):
        raise AssertionError("device touched")
    monkeypatch.setattr(_native, "Context", touched)
    monkeypatch.setattr(_native, "default_context", touched)


def test_session_checks_x_meas_before_any_device_work(monkeypatch):
    from trajoptmpcreference_amd import MPCSession
    _no_device(monkeypatch)
    B, N = 4, 8
    s = fixed_solver("arm3").MPC_session(np.zeros((B, 6, N)), np.zeros((B, 3, N - 1)), N, 0.1, "QP-PCG-SS")
    assert isinstance(s, MPCSession)
    for bad in (np.zeros((B, 5)), np.zeros((B + 1, 6)), np.zeros(6), np.zeros((B, 6, 1))):
        with pytest.raises(ValueError, match=r"x_meas must be \[B\]\[nx\] = \(4, 6\)"):
            s.step(bad)
    with pytest.raises((ValueError, TypeError)):
        s.step([["a"] * 6] * B)
    assert s.steps_done == 0
    x, u = s.horizon()   # nothing ran: the horizon it was given
    assert x.shape == (B, 6, N) and u.shape == (B, 3, N - 1) and s.soft_state() is None
    s.close()
    with pytest.raises(RuntimeError, match="closed"):
        s.step()


def test_session_checks_its_arguments_before_any_device_work(monkeypatch):
    _no_device(monkeypatch)
    s = fixed_solver("arm3")
    B, N = 2, 8
    x, u = np.zeros((B, 6, N)), np.zeros((B, 3, N - 1))
    with pytest.raises(ValueError, match="expected x"):
        s.MPC_session(x[:, :5], u, N, 0.1)
    with pytest.raises(ValueError, match="expected x"):
        s.MPC_session(x, u, N + 1, 0.1)
    with pytest.raises(NotImplementedError, match="MPC solver"):
        s.MPC_session(x, u, N, 0.1, "QP-XYZ")
    with pytest.raises(ValueError, match="goal must be"):
        s.MPC_session(x, u, N, 0.1, goal=np.zeros((B, 7)))
    with pytest.raises(ValueError, match="R = 3 rows"):
        s.MPC_session(x, u, N, 0.1, goal=np.zeros((3, 6, N)))


def test_session_refuses_urdf_cost_and_plugin_hooks(monkeypatch):
    from trajoptmpcreference_amd import QuadraticCost, TrajoptMPCReference, UrdfCost
    _no_device(monkeypatch)
    p = plant("arm2")
    x, u = np.zeros((2, 4, 4)), np.zeros((2, 2, 3))
    s = TrajoptMPCReference(p, UrdfCost(p, np.eye(4), np.eye(4), np.eye(2), np.zeros(4)))
    with pytest.raises(NotImplementedError, match="QuadraticCost only"):
        s.MPC_session(x, u, 4, 0.1)

    class Mine(QuadraticCost):   # a caller's own hook: the plugin-hook path, which has no MPC loop
        def value(self, *a, **k):
            return 0.0
    s = TrajoptMPCReference(p, Mine(np.eye(4), np.eye(4), np.eye(2), np.zeros(4)))
    with pytest.raises(NotImplementedError, match="device plugins only"):
        s.MPC_session(x, u, 4, 0.1)
