"""CPU: pin oracle/qp_hp.py (the QP in long double, the reference of test_gpu_qp_kernels.py) and the inputs of
tests/qp_cases.py.

* Against the reference's own QP fixtures (tests/golden/qp_*.npz): S, gamma within those fixtures' tolerance of
  test_oracle_golden.py (1e-11), lam_direct within test_gpu_pcg.py's 1e-9, and the fixtures' dxul_direct leaves a
  long-double KKT residual at rounding level: a backward-stable solve of n = N nx <= 384 rows leaves a normwise
  residual of order n eps = 4e-14, the bound is 1e-13.
* Against oracle/sqp.py in fp64 on the groups of qp_cases (cut to 2 problems; arm1 at N = 2, arm12 at N = 4):
  schur_blocks is schur_hp to rounding.  S and gamma are inner products of length nx + nu <= 36 nested twice
  through an inverse of condition <= 1e3 that is exact when diagonal: the bound is 256 * 2^-53 = 2.8e-14 of
  max|ref|; on the soft groups, whose G_k carry mu-weighted outer products, times the largest condition number
  of a G_k + rho I (an input property).  dxu = Ghat (g - C^T lambda) is printed, not bound: the difference
  cancels (lambda is of QF's size), 9e-14 here on the default cost.  MEASURED here without soft limits:
  Ghat <= 5.6e-16, S <= 8.9e-16, gamma <= 3.0e-15; soft groups: Ghat 7.7e-15, gamma 1.2e-13 at condition 4e3.
* Every sample is informative: c_0 != 0, some c_k != 0 with k >= 1, g != 0, lambda != 0; the soft groups
  violate a limit at two knots or more.
* Sensitivity: the structural errors the dense groups exist to catch, applied to the fp64 candidate, push it past
  test_gpu_qp_kernels.py's bound (8 err_cpu64 + 4 * 2^-53) where the cost is dense and pass unnoticed on the
  default cost.  MEASURED here, err / bound on arm6 N = 8 (the test prints every figure): a wrong sub-block
  4e11 .. 2e14, Ghat_u of the wrong knot 1.7e15 (soft group), Q for QF 6.7e13, the goal dropped 5e11 .. 1.4e14,
  one entry of Ghat off by 1e-9 of itself 73 (rho = 1e3) .. 9.8e4; on the default cost every one of the first
  four stays at 0.1 (no change at all).
  Two findings about the list of errors itself:
    - "Ghat_x transposed" is invisible on EVERY symmetric cost, dense or not: Ghat_x is symmetric to rounding
      (asserted here), so a transposed Ghat index cannot be caught by any quadratic cost the solver accepts.  The
      nearest error a dense cost does catch is a wrong sub-block -- the q and qd diagonal sub-blocks of Ghat_x
      swapped inside S_lo -- and that one is in the list.
    - "Ghat_u from the wrong knot" is invisible without soft limits on every cost: R is one block for all knots.
      It shows on the soft groups (per-knot Ghat_u from k_ginv_soft), which is where it is asserted.
"""
import numpy as np
import pytest

import qp_cases as qc
from conftest import arm_model, golden, quad_cost_arrays
from ilqr_cases import violated
from oracle import qp_hp
from oracle import sqp as osqp

assert np.finfo(np.longdouble).eps < 2e-19, "long double is not an extended-precision format on this host"

EPS = 2.0 ** -53
CPU_BOUND = 256 * EPS
CPU_MODELS = ["arm1", "arm3", "arm6", "arm7", "tree4", "arm12"]


def _rel1(a, b):
    """test_oracle_golden.py's measure: relative to max(1, max|b|)"""
    return float(np.max(np.abs(np.asarray(a, dtype=qc.HP) - np.asarray(b, dtype=qc.HP)))) / max(1.0, float(np.max(np.abs(b))))


# ------------------------------------------------------------------------------------------------ fixtures
@pytest.mark.parametrize("name,N", [("arm2", 8), ("arm3", 32), ("arm6fix", 64)])
def test_qp_hp_matches_reference_fixtures(name, N):
    d = golden(f"qp_{name}_N{N}.npz")
    m = arm_model(name)
    nx, nu = 2 * m.n, m.n
    cost = osqp.QuadCost(*quad_cost_arrays(m.n))
    x, u, rho = d["x"], d["u"], float(d["rho"])
    G, g, A, B, c = osqp.kkt_blocks(m, cost, x, u, x[:, 0].copy(), N, float(d["dt"]))
    Gh, Sd, Sl, gam = qp_hp.schur_hp(G, g, A, B, c, rho, nx)
    assert _rel1(Sd, d["S_diag"]) < 1e-11 and _rel1(Sl, d["S_lo"]) < 1e-11
    assert _rel1(gam.reshape(-1), d["gamma"]) < 1e-11
    lam = qp_hp.solve_hp(Sd, Sl, gam)
    assert qp_hp.backward_error(Sd, Sl, gam, lam) < 1e-18   # the elimination itself, in long double
    e_lam = _rel1(lam.reshape(-1), d["dxul_direct"][-N * nx:])
    print(f"{name} N={N}: lam_direct against solve_hp {e_lam:.3e}")
    assert e_lam < 1e-9
    # the fixture's own direct solution in the long-double KKT system: (G + rho I) dz + C^T lam = g, C dz = c
    dz, lf = qp_hp.hp(d["dxul_direct"][:-N * nx]), qp_hp.hp(d["dxul_direct"][-N * nx:]).reshape(N, nx)
    n = nx + nu
    r1 = r2 = s1 = s2 = qc.HP(0)
    for k in range(N):
        w = n if k < N - 1 else nx
        z = dz[n * k:n * k + w]
        Gr = qp_hp.hp(G[k]) + qc.HP(rho) * np.eye(w, dtype=qc.HP)
        ctl = lf[k].copy() if k == N - 1 else np.concatenate([lf[k] - qp_hp.hp(A[k]).T @ lf[k + 1],
                                                              -qp_hp.hp(B[k]).T @ lf[k + 1]])
        r1 = max(r1, np.max(np.abs(Gr @ z + ctl - qp_hp.hp(g[k]))))
        s1 = max(s1, np.max(np.abs(Gr)) * np.max(np.abs(z)) + np.max(np.abs(ctl)) + np.max(np.abs(g[k])))
        cz = z[:nx].copy()
        if k > 0:
            zp = dz[n * (k - 1):n * k]
            cz -= qp_hp.hp(A[k - 1]) @ zp[:nx] + qp_hp.hp(B[k - 1]) @ zp[nx:]
        r2 = max(r2, np.max(np.abs(cz - qp_hp.hp(c[k]))))
    # C dz - c = gamma - S lam identically (dz = Ghat (g - C^T lam)): the feasibility residual is the Schur
    # solve's, so its scale is that system's |S| |lam| + |gamma|
    rows = np.sum(np.abs(Sd), axis=2)
    rows[1:] += np.sum(np.abs(Sl), axis=2)
    rows[:-1] += np.sum(np.abs(Sl), axis=1)
    s2 = np.max(rows) * np.max(np.abs(lf)) + np.max(np.abs(gam))
    print(f"{name} N={N}: KKT residuals of dxul_direct: stationarity {float(r1 / s1):.3e}, feasibility {float(r2 / s2):.3e}")
    assert float(r1 / s1) < 1e-13 and float(r2 / s2) < 1e-13


def test_inv_hp_and_solve_hp_on_known_answers():
    rng = np.random.default_rng(3)
    M = rng.standard_normal((9, 9))
    Mi = qp_hp.inv_hp(M)
    assert float(np.max(np.abs(Mi @ qp_hp.hp(M) - np.eye(9)))) < 1e-16
    assert float(np.max(np.abs(Mi - np.linalg.inv(M)))) < 1e-11
    # a leading zero needs the pivot search
    P = np.array([[0.0, 2.0], [4.0, 1.0]])
    assert float(np.max(np.abs(qp_hp.inv_hp(P) - np.linalg.inv(P)))) < 1e-16
    # block-tridiagonal solve against the dense one
    N, nx = 5, 3
    Sd = np.array([-(np.eye(nx) * 4 + 0.1 * rng.standard_normal((nx, nx))) for _ in range(N)])
    Sd = 0.5 * (Sd + np.transpose(Sd, (0, 2, 1)))
    Sl = 0.5 * rng.standard_normal((N - 1, nx, nx))
    gam = rng.standard_normal((N, nx))
    lam = qp_hp.solve_hp(Sd, Sl, gam)
    ref = np.linalg.solve(osqp.dense_from_blocks(Sd, Sl, np.transpose(Sl, (0, 2, 1))), gam.reshape(-1))
    assert float(np.max(np.abs(lam.reshape(-1) - ref))) < 1e-13
    assert float(np.max(np.abs(qp_hp.residual_hp(Sd, Sl, gam, lam)))) < 1e-17
    Pd = qp_hp.precond_diag_hp(Sd)
    assert float(np.max(np.abs(Pd - np.linalg.inv(Sd)))) < 1e-14


# ------------------------------------------------------------------------------------------------ the groups
def _cpu_group(g):
    """a group at the size this file runs it: 2 problems; arm1 at N = 2, arm12 at N = 4"""
    N = min(g.N, qc.cpu_sizes(g.model))
    return g._replace(N=N, B=2)


def _cpu_groups(key):
    return sorted({_cpu_group(g) for g in qc.groups_of(key)}, key=qc.gid)


@pytest.mark.parametrize("key", CPU_MODELS)
def test_fp64_oracle_is_qp_hp_to_rounding_and_samples_are_informative(key):
    nx = 2 * qc.model(key).n
    for g in _cpu_groups(key):
        x, u, xs = qc.problems(g.model, g.N, g.B, g.seed)
        viol = 0
        for b in range(g.B):
            G, gg, A, B, c = qc.kkt(g, b)
            assert np.max(np.abs(c[0])) > 0 and np.max(np.abs(c[1:])) > 0, (qc.gid(g), b, "a defect vanishes")
            assert all(np.max(np.abs(gk)) > 0 for gk in gg), (qc.gid(g), b, "a zero gradient")
            rho = float(qc.rhos(g)[b])
            Gh, Sd, Sl, gam = qp_hp.schur_hp(G, gg, A, B, c, rho, nx)
            Gh64, Sd64, Sl64, gam64 = osqp.schur_blocks(G, gg, A, B, c, rho, nx)
            lam = qp_hp.solve_hp(Sd, Sl, gam)
            assert np.min(np.max(np.abs(lam), axis=1)) > 0, (qc.gid(g), b, "a zero multiplier block")
            eS = max(qc.rel(Sd64, Sd), qc.rel(Sl64, Sl))
            eg = qc.rel(gam64, gam)
            eG = max(qc.rel(a, r) for a, r in zip(Gh64, Gh))
            dxu = qp_hp.dxu_hp(Gh, gg, A, B, lam, nx)
            e_d = qc.rel(osqp.recover_dxu(Gh64, gg, A, B, np.asarray(lam, dtype=float).reshape(-1), nx)[:dxu.size], dxu)
            # soft limits add mu-weighted outer products to G_k: the inverse's error grows with its condition
            kappa = max(np.linalg.cond(Gk + rho * np.eye(len(Gk))) for Gk in G) if g.soft != "none" else 1.0
            print(f"{qc.gid(g)} b={b}: err_cpu64 Ghat {eG:.2e} S {eS:.2e} gamma {eg:.2e} dxu {e_d:.2e} "
                  f"(cond {kappa:.1e})")
            assert max(eG, eS, eg) <= CPU_BOUND * kappa, (qc.gid(g), b, eG, eS, eg, kappa)
            viol += violated(g.soft, x[b], u[b]) if g.soft != "none" else 0
        if g.soft != "none":
            assert viol >= 2, (qc.gid(g), viol)


def test_case_layout():
    """what section 3 of the cases promises"""
    for key in qc.FULL_MODELS + qc.WIDE_MODELS:
        gs = qc.groups_of(key)
        assert {g.N for g in gs} >= {2, 3, 8}
        assert {g.cost for g in gs} == {"default", "identity", "dense", "qfstart", "qfstart-dense"}
        for c in ("default", "identity", "dense"):   # every rho with every cost and with every horizon
            assert {g.rho for g in gs if g.cost == c and g.B == 8 and g.soft == "none"} == set(qc.RHOS)
        for N in (2, 3, 8):
            assert {g.rho for g in gs if g.N == N and g.B == 8 and g.soft == "none" and g.cost in
                    ("default", "identity", "dense")} == set(qc.RHOS)
        if key in qc.WIDE_MODELS:
            assert all(g.soft == "none" for g in gs)
        else:
            assert {(g.cost, g.soft) for g in gs if g.soft != "none"} == {
                ("default", "torque"), ("dense", "joint+torque"), ("dense", "torque"), ("default", "joint+torque")}
    assert [g.model for k in ("arm3", "arm6", "arm12") for g in qc.groups_of(k) if g.B == 65] == ["arm3", "arm6", "arm12"]
    assert sum(g.B == 1 for k in qc.FULL_MODELS for g in qc.groups_of(k)) == 1
    Q, QF, R, xg, qfs = qc.cost_arrays("qfstart-dense", 3, 8)
    assert qfs == 4 and np.max(np.abs(Q - np.diag(np.diag(Q)))) > 0.01 and np.max(np.abs(Q - QF)) > 0.01
    rows = {k: g.N * 2 * qc.model(g.model).n for k, (g, _) in qc.INSTANCES.items()}
    assert rows["two-rows-arm7"] == 770 and rows["two-rows-arm12"] == 792 and rows["gm-natural"] == 1032


# ------------------------------------------------------------------------------------------------ sensitivity
def _candidate(g, b, mutation=None):
    """schur_blocks of oracle/sqp.py in fp64 with one structural error; (Ghat_x, Ghat_u, Sd, Sl, gam)"""
    G, gg, A, B, c = qc.kkt(g, b)
    N, nx = g.N, A.shape[1]
    rho = float(qc.rhos(g)[b])
    cost = qc.quad_cost(g)
    x, u, _ = qc.problems(g.model, g.N, g.B, g.seed)
    G, gg = [Gk.copy() for Gk in G], [gk.copy() for gk in gg]
    if mutation == "q-for-qf":      # Q where QF_start says QF (the terminal knot keeps QF)
        for k in range(N - 1):
            if cost.QF_start is not None and k >= cost.QF_start:
                G[k][:nx, :nx] += cost.Q - cost.QF
                gg[k][:nx] += (x[b][:, k] - cost.xg) @ (cost.Q - cost.QF)
    if mutation == "no-goal":       # xg dropped from the gradient
        for k in range(N):
            gg[k][:nx] += cost.xg @ cost.currQ(k == N - 1, k)
    Gh = [np.linalg.inv(Gk + rho * np.eye(len(Gk))) for Gk in G]
    if mutation == "entry":         # one entry of Ghat off by 1e-9 of itself
        Gh[N // 2][1, 0] *= 1 + 1e-9
    Ghu = [Gk[nx:, nx:] for Gk in Gh[:-1]]
    if mutation == "u-knot":        # Ghat_u from the next knot's block
        Ghu = Ghu[1:] + Ghu[:1]
    Sd, Sl, gam = np.zeros((N, nx, nx)), np.zeros((N - 1, nx, nx)), np.zeros((N, nx))
    Sd[0] = -Gh[0][:nx, :nx]
    gam[0] = c[0] - (Gh[0] @ gg[0])[:nx]
    nj = nx // 2
    for k in range(N - 1):
        Gx = Gh[k][:nx, :nx]
        Sd[k + 1] = -(A[k] @ Gx @ A[k].T + B[k] @ Ghu[k] @ B[k].T + Gh[k + 1][:nx, :nx])
        Gl = Gx
        if mutation == "transpose":
            Gl = Gx.T
        if mutation == "sub-block":   # the q and qd diagonal sub-blocks swapped
            Gl = Gx.copy()
            Gl[:nj, :nj], Gl[nj:, nj:] = Gx[nj:, nj:], Gx[:nj, :nj]
        Sl[k] = A[k] @ Gl
        gam[k + 1] = c[k + 1] + A[k] @ (Gx @ gg[k][:nx]) + B[k] @ (Ghu[k] @ gg[k][nx:]) - (Gh[k + 1] @ gg[k + 1])[:nx]
    return np.array([Gk[:nx, :nx] for Gk in Gh]), np.array(Ghu), Sd, Sl, gam


def _excess(g, mutation):
    """the largest err / (8 err_cpu64 + floor) over Ghat, S, gamma and the group's problems: > 1 is caught"""
    nx = 2 * qc.model(g.model).n
    worst = 0.0
    for b in range(g.B):
        G, gg, A, B, c = qc.kkt(g, b)
        Gh, Sd, Sl, gam = qp_hp.schur_hp(G, gg, A, B, c, float(qc.rhos(g)[b]), nx)
        Gx, Gu = qc.blocks(Gh, nx)
        base, cand = _candidate(g, b), _candidate(g, b, mutation)
        for got, b64, ref in zip(cand, base, (Gx, Gu, Sd, Sl, gam)):
            worst = max(worst, qc.rel(got, ref) / (qc.MARGIN64 * qc.rel(b64, ref) + qc.FLOOR))
    return worst


DEFAULT = qc.Group("arm6", 8, "default", "none", 2, 600, 1.0)
DENSE = qc.Group("arm6", 8, "dense", "none", 2, 600, 1.0)
DENSE_QFS = qc.Group("arm6", 8, "qfstart-dense", "none", 2, 621, 1.0)
DENSE_SOFT = qc.Group("arm6", 8, "dense", "joint+torque", 2, 680, 1e-3)
DENSE_HI = qc.Group("arm6", 8, "dense", "none", 2, 600, 1e3)
# mutation -> the dense groups that must catch it
MUTATIONS = {
    "sub-block": [DENSE, DENSE_QFS, DENSE_SOFT, DENSE_HI],
    "u-knot": [DENSE_SOFT],
    "q-for-qf": [DENSE_QFS],
    "no-goal": [DENSE, DENSE_QFS, DENSE_SOFT, DENSE_HI],
    "entry": [DENSE, DENSE_QFS, DENSE_SOFT, DENSE_HI],
}


def test_the_unmutated_candidate_is_within_the_bound():
    for g in (DEFAULT, DENSE, DENSE_QFS, DENSE_SOFT, DENSE_HI):
        assert _excess(g, None) <= 1.0, qc.gid(g)


@pytest.mark.parametrize("mutation", list(MUTATIONS))
def test_dense_groups_catch_a_structural_error(mutation):
    for g in MUTATIONS[mutation]:
        e = _excess(g, mutation)
        print(f"{mutation} on {qc.gid(g)}: err / bound = {e:.3g}")
        assert e > 1.0, (mutation, qc.gid(g), e)


@pytest.mark.parametrize("mutation", ["transpose", "sub-block", "u-knot", "q-for-qf", "no-goal"])
def test_the_default_cost_does_not_notice(mutation):
    """the point of the dense groups: on the suite's default cost (Ghat a scalar multiple of I per block, goal
    0, no QF_start) the structural errors change nothing"""
    e = _excess(DEFAULT, mutation)
    print(f"{mutation} on {qc.gid(DEFAULT)}: err / bound = {e:.3g}")
    assert e <= 1.0, (mutation, e)


def test_a_transposed_ghat_is_invisible_on_every_symmetric_cost():
    """Ghat_x is symmetric to rounding, so transposing it inside S_lo stays inside the bound on the dense groups
    too (see the module docstring): no symmetric cost can catch a transposed Ghat index"""
    for g in (DENSE, DENSE_QFS, DENSE_SOFT, DENSE_HI):
        for b in range(g.B):
            Gx = _candidate(g, b)[0]
            assert np.max(np.abs(Gx - np.transpose(Gx, (0, 2, 1)))) <= 4 * EPS * np.max(np.abs(Gx)), qc.gid(g)
        e = _excess(g, "transpose")
        print(f"transpose on {qc.gid(g)}: err / bound = {e:.3g}")
        assert e <= 1.0, (qc.gid(g), e)
