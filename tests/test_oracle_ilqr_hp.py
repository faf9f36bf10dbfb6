"""The inputs of the iLQR kernel tests (tests/ilqr_cases.py), checked on the CPU: not the kernel.

The GPU tests bound the Riccati kernels' error by a small multiple of the error a CPU sweep of the same
precision makes against the extended-precision sweep (oracle/ilqr.py backward_hp, long double).  That is a
meaningful bound only where the CPU sweeps are themselves accurate, so on every case group:
  * the fp64 sweep (oilqr.backward, the canonical order) is within 1e-9 of backward_hp;
  * on the groups used for fp32, the float32 sweep (backward_hp with dtype = float32) is within 5e-4.
Errors are max|a - ref| / max(1, max|ref|), separately for K, d and (dV1, dV2).  Measured with these caps'
margins: seeds 500..507, N = 8..32, rho = 1e-3: the default cost (QF = 100 I, R = 0.1 I) up to 1.0e-10 in
fp64 and up to 1e-1 in fp32 on arm6 (Q_uu's condition is ~1e5: no fp32 group uses it); Q = QF = R = I
<= 2.4e-13 / 8.3e-5; dense SPD blocks with eigenvalues in [0.5, 2] <= 2.4e-13 / 1.4e-4; smaller at rho = 1
and 1e3.
"""
import numpy as np
import pytest

import ilqr_cases as cases
from oracle import ilqr as oilqr

# the reference's format: x87 extended precision (64-bit significand)
assert np.finfo(np.longdouble).eps < 2e-19, "long double is not an extended-precision format on this host"

CAP64, CAP32 = 1e-9, 5e-4


@pytest.mark.parametrize("key", cases.FULL_MODELS + cases.WIDE_MODELS)
def test_fp64_sweep_is_close_to_extended_precision(key):
    for g in cases.groups_of(key):
        A, Bm = cases.cpu_jacobians(g)
        errs = cases.sweep_errors(g, A, Bm, {"cpu64": cases.cpu64_sweep})
        for rho, e in errs.items():
            for what, v in e["cpu64"].items():
                assert v <= CAP64, (cases.gid(g), rho, what, v)


@pytest.mark.parametrize("key", cases.F32_MODELS)
def test_fp32_sweep_is_close_to_extended_precision(key):
    for g in cases.f32_groups_of(key):
        A, Bm = cases.cpu_jacobians(g)
        errs = cases.sweep_errors(g, A, Bm, {"cpu32": cases.cpu32_sweep})
        for rho, e in errs.items():
            for what, v in e["cpu32"].items():
                assert v <= CAP32, (cases.gid(g), rho, what, v)


def test_backward_hp_restates_backward():
    """backward_hp in float64 is the recursion of `backward` up to the order of its sums (numpy's `@` against
    chol_solve's sequential loops): the two agree to rounding, and both refuse an indefinite Q_uu."""
    g = cases.Group("arm3", 8, "dense", "joint+torque", 8, 580, "mixed")
    A, Bm = cases.cpu_jacobians(g)
    for b, rho in enumerate(cases.rhos(g)):
        dv = cases.derivatives(g, b)
        K, d, dV1, dV2, ok = oilqr.backward(A[b], Bm[b], *dv, rho)
        hp = oilqr.backward_hp(A[b], Bm[b], *dv, rho, dtype=np.float64)
        assert ok and hp is not None
        assert hp[0].dtype == np.float64
        assert cases.rel_err(hp[0], np.array(K)) < 1e-12 and cases.rel_err(hp[1], np.array(d)) < 1e-12
        assert cases.rel_err([hp[2], hp[3]], [dV1, dV2]) < 1e-12
    dv = cases.derivatives(g, 0)
    assert oilqr.backward_hp(A[0], Bm[0], *dv, -1e3) is None
    assert oilqr.backward(A[0], Bm[0], *dv, -1e3)[4] is False


def test_soft_groups_violate_their_limits():
    """every soft-limit group has a knot past each of its limits, so the sweeps see non-zero jacobian terms"""
    for key in cases.FULL_MODELS:
        for g in cases.groups_of(key):
            if g.soft == "none":
                continue
            x, u = cases.problems(g.model, g.N, g.B, g.seed)
            n = u.shape[1]
            assert sum(cases.violated(g.soft, x[b], u[b]) for b in range(g.B)) > 0, cases.gid(g)
            assert np.any(np.abs(u) > cases.SOFT_BOUNDS["torque"]), cases.gid(g)
            if "joint" in cases.SOFT_KINDS[g.soft]:
                assert np.any(np.abs(x[:, :n]) > cases.SOFT_BOUNDS["joint"]), cases.gid(g)
