"""Inputs shared by the QP kernel-level tests (test_oracle_qp_hp.py on the CPU, test_gpu_qp_kernels.py on the
GPU): the case groups, their problems, costs, soft state and the error measures.  Built on tests/ilqr_cases.py
(models, costs, RHOS, the soft bounds, the group tuple (model, N, cost, soft, B, seed, rho)).

Problems.  The iLQR cases are rollouts: their defects c_k vanish for k >= 1, which leaves half of gamma
untested.  A QP problem starts from osqp.initial_problem(model, N, DT, seed + b) and takes, all from
default_rng(seed + b): u ~ U(-0.2, 0.2), x += U(-0.05, 0.05) on every knot, xs = x[:, 0] + U(-0.05, 0.05).
test_oracle_qp_hp.py asserts that every sample is informative (c_0 != 0, some c_k != 0 for k >= 1, g != 0,
lambda != 0).

Costs: ilqr_cases.cost_arrays' kinds and "qfstart-dense", the dense blocks (QF != Q) with QF_start inside the
horizon -- a Q / QF swap at a QF_start knot is invisible when only the terminal knot differs.

Soft groups carry a non-trivial soft state, mu ~ U(1, 10) and lambda ~ U(0, 1) per knot and slot, set on the
device right before each call and mirrored into the oracle's SoftLimit.mu / .lam.

Errors are max|a - ref| / max|ref| in long double, NOT floored at 1: at rho = 1e3 Ghat is about 1e-3 and
ilqr_cases.rel_err's floor would hide an error there.
"""
import functools

import numpy as np

import ilqr_cases as cases
from ilqr_cases import DT, HP, RHOS, Group, gid, model, rhos  # noqa: F401  (re-exported)
from oracle import qp_hp
from oracle import sqp as osqp
from oracle.soft import TYPES

MARGIN64 = 8.0            # test_gpu_ilqr_kernels.py's
FLOOR = 4 * 2.0 ** -53    # a correctly rounded CPU result against a valid other order: an ulp or two


def cost_arrays(kind, n, N):
    if kind == "qfstart-dense":
        Q, QF, R, xg, _ = cases.cost_arrays("dense", n, N)
        assert not np.allclose(Q, QF)
        return Q, QF, R, xg, N // 2
    return cases.cost_arrays(kind, n, N)


def quad_cost(g):
    Q, QF, R, xg, qfs = cost_arrays(g.cost, model(g.model).n, g.N)
    return osqp.QuadCost(Q, QF, R, xg, qfs)


@functools.lru_cache(maxsize=None)
def problems(key, N, B, seed):
    """x [B][nx][N], u [B][nu][N-1], xs [B][nx] (read-only: shared between tests)"""
    m = model(key)
    xs_, us_, x0_ = [], [], []
    for b in range(B):
        x, u = osqp.initial_problem(m, N, DT, seed + b)
        rng = np.random.default_rng(seed + b)
        u = rng.uniform(-0.2, 0.2, u.shape)
        x = x + rng.uniform(-0.05, 0.05, x.shape)
        x0_.append(x[:, 0] + rng.uniform(-0.05, 0.05, x.shape[0]))
        xs_.append(x)
        us_.append(u)
    out = np.array(xs_), np.array(us_), np.array(x0_)
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def soft_state(g):
    """(mu, lam) [B][N][6n] of a soft group (None, None otherwise)"""
    if g.soft == "none":
        return None, None
    n = model(g.model).n
    rng = np.random.default_rng(g.seed + 7919)
    mu = rng.uniform(1.0, 10.0, (g.B, g.N, 6 * n))
    lam = rng.uniform(0.0, 1.0, (g.B, g.N, 6 * n))
    mu.setflags(write=False)
    lam.setflags(write=False)
    return mu, lam


def soft_oracle(g, b):
    """the oracle's soft limits of problem b, at the group's soft state"""
    n = model(g.model).n
    soft = cases.soft_oracle(g.soft, n, g.N)
    if soft is None:
        return None
    mu, lam = soft_state(g)
    for lim in soft.limits:
        t = TYPES.index(lim.kind)
        lim.mu = mu[b, :lim.T, t * 2 * n:(t + 1) * 2 * n].T.copy()
        lim.lam = lam[b, :lim.T, t * 2 * n:(t + 1) * 2 * n].T.copy()
    return soft


@functools.lru_cache(maxsize=None)
def kkt(g, b):
    """G, g (per-knot lists), A, B, c of problem b: osqp.kkt_blocks (the oracle's dynamics)"""
    x, u, xs = problems(g.model, g.N, g.B, g.seed)
    return osqp.kkt_blocks(model(g.model), quad_cost(g), x[b], u[b], xs[b], g.N, DT, soft_oracle(g, b))


def rel(a, ref):
    """max|a - ref| / max|ref| in long double (no floor)"""
    ref = np.asarray(ref, dtype=HP)
    return float(np.max(np.abs(np.asarray(a, dtype=HP) - ref)) / np.max(np.abs(ref)))


def blocks(Gh, nx):
    """a per-knot Ghat list as (Ghat_x [N][nx][nx], Ghat_u [N-1][nu][nu])"""
    return np.array([G[:nx, :nx] for G in Gh]), np.array([G[nx:, nx:] for G in Gh[:-1]])


_GHAT = {}


def ghat_ref(g, b):
    """inv_hp(G_k + rho I) per knot, long double; one inversion per distinct block (without soft limits a
    group has two per rho)"""
    rho = float(rhos(g)[b])
    out = []
    for Gk in kkt(g, b)[0]:
        key = (Gk.shape[0], rho, Gk.tobytes())
        if key not in _GHAT:
            _GHAT[key] = qp_hp.ghat_hp([Gk], rho)[0]
            _GHAT[key].setflags(write=False)
        out.append(_GHAT[key])
    return out


def picked(g):
    """the problems whose S, gamma, P and dxu are compared: all of them, or 24 of a batch of 65 (8 per rho; both
    sides of the 32- and 64-problem boundaries) -- Ghat is compared for every problem"""
    return list(range(g.B)) if g.B <= 8 else list(range(0, 8)) + list(range(28, 36)) + list(range(57, 65))


def cpu64_schur(g, b, A, Bm, c):
    """the fp64 oracle on the given A, Bm, c and the group's cost blocks: (Gh, Sd, Sl, gam)"""
    G, gg = kkt(g, b)[:2]
    return osqp.schur_blocks(G, gg, A, Bm, c, float(rhos(g)[b]), A.shape[1])


# ------------------------------------------------------------------------------------------------ the groups
FULL_MODELS = cases.FULL_MODELS
WIDE_MODELS = cases.WIDE_MODELS
DENSE = ("dense", "qfstart-dense")


def groups_of(key):
    """the groups of one model: horizons 2, 3, 8 x costs default, identity, dense with the three rho as a Latin
    square (ilqr_cases.groups_of), both QF_start costs, B = 1 once (arm3), B = 65 with mixed rho (arm3, arm6,
    arm12: 195 matrices, not a multiple of the 4 or 2 a wave of k_ginv holds at 16 or 32 lanes per matrix), the soft groups"""
    grid = [(N, c) for N in (2, 3, 8) for c in ("default", "identity", "dense")]
    gs = [Group(key, N, c, "none", 8, 600, RHOS[(i + i // 3) % 3]) for i, (N, c) in enumerate(grid)]
    gs += [Group(key, 8, "qfstart", "none", 8, 620, 1e-3), Group(key, 8, "qfstart-dense", "none", 8, 621, 1.0)]
    if key in ("arm3", "arm6", "arm12"):
        gs.append(Group(key, 8, "dense", "none", 65, 640, "mixed"))
    if key == "arm3":
        gs.append(Group(key, 8, "dense", "none", 1, 641, 1e-3))
    if key in FULL_MODELS:
        gs += [Group(key, 8, "default", "torque", 8, 650, 1.0), Group(key, 8, "dense", "joint+torque", 8, 680, 1e-3),
               Group(key, 3, "dense", "torque", 8, 670, 1.0), Group(key, 2, "default", "joint+torque", 8, 660, 1e3)]
    return gs


def cpu_sizes(key):
    """the sizes test_oracle_qp_hp.py runs a model's groups at: arm1 N = 2; arm12 N = 4; the others N = 8 (the
    rest of each group unchanged; batches cut to 2)"""
    return {"arm1": 2, "arm12": 4}.get(key, 8)


# instance shapes: each the smallest that reaches the instance; B = 2, dense cost, mixed rho.  (group, the
# TMPC_QP_GM_MIN_ROWS to force or None)
INSTANCES = {
    "one-row": (Group("arm3", 8, "dense", "none", 2, 700, "mixed"), None),
    "two-rows-arm7": (Group("arm7", 55, "dense", "none", 2, 701, "mixed"), None),     # 770 rows
    "two-rows-arm12": (Group("arm12", 33, "dense", "none", 2, 702, "mixed"), None),   # 792 rows
    "gm-forced-arm3": (Group("arm3", 8, "dense", "none", 2, 700, "mixed"), 1),
    "gm-forced-arm1": (Group("arm1", 2, "dense", "none", 2, 703, "mixed"), 1),
    "gm-natural": (Group("arm6", 86, "dense", "none", 2, 704, "mixed"), None),        # 1032 rows
}
