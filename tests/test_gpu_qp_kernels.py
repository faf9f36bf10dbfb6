"""Unit parity of the QP kernels (k_ginv at 16 and at 32 lanes per matrix, k_ginv_soft, k_qp's prologue qp_schur_row, its
preconditioner, PCG and epilogue, k_btsolve) through tmpc_qp_batch and tmpc_qp_last_inputs, which reads back what
the QP consumed: A, Bm, c and the per-knot Ghat.  Inputs: tests/qp_cases.py (conditioned and shown to be
sensitive on the CPU by test_oracle_qp_hp.py): dense costs, non-zero goals, QF_start with dense QF != Q, 1..12
joints and the tree, soft limits at a non-trivial state, mixed rho inside a batch, batches of 65.

Reference: oracle/qp_hp.py in long double on the GPU's OWN A, Bm, c (so the dynamics' rounding is not in S; A,
Bm, c themselves are held to the oracle's at test_gpu_dynamics.py's 1e-12, and to a long-double reference on
general robots by test_gpu_dynamics_hp.py) and on the cost's G, g.  Errors are
max|a - ref| / max|ref| (not floored at 1), the largest over the problems of a group that share a rho.  Bound,
per quantity:  err_gpu <= 8 err_cpu64 + 4 * 2^-53,  err_cpu64 from the fp64 oracle (np.linalg.inv, schur_blocks,
recover_dxu) on the same inputs; the floor covers a CPU result that is correctly rounded (a diagonal inverse)
against a kernel that multiplies by a reciprocal (gj_pivot: two roundings where a division has one).
  Ghat_x, Ghat_u   against inv_hp(G_k + rho I);
  S_diag, S_lo, gamma   against schur_hp (which forms Ghat itself: an error in Ghat shows here too);
  P_diag (BJ, SS)  against precond_diag_hp on the GPU's own S_diag, np.linalg.inv as the fp64 candidate;
  direct methods   the normwise backward error |S lam - gamma| / (|S| |lam| + |gamma|) on the GPU's own S, gamma
                   against 8 x np.linalg.solve's on the dense S (cond(S) reaches 3e8: a forward-error ratio of an
                   unpivoted block elimination to LAPACK would not be a fair test; the forward error against
                   solve_hp is printed); methods N and S give the same bits;
  epilogue         the x, u part of dxul against dxu_hp with the GPU's own lambda, for PCG-SS and S.
PCG on the dense groups: count and lambda are bit for bit oracle/canon.c's on the GPU's own S, gamma, in the lane
layout the instance ran, for all four preconditioners, mixed rho, both register layouts, the GM instance forced
and natural, and with a warm start.
Bitwise relations: a problem alone against itself at positions 0, 31, 64 of a batch of 65; S, gamma and the
read-back from the one-row instance, the forced GM instance and method S's SCHUR-mode prologue; diagonal blocks
through the fast path against TMPC_GENERIC_COST=1; a constant reference equal to xg against the fixed goal.

Hard limits on a dense cost (ACTIVE_SET torque + velocity at +-2.0, arm3 and arm6 N = 8, B = 4): active sets and
dimension are oracle/hard.py's, S_band and gamma at test_gpu_hard.py's 1e-10, pcg_canonical on the GPU's own band
gives the GPU's count and lambda bit for bit.

Every figure is printed; each test raises its largest ratio as a warning (as test_gpu_ilqr_kernels.py).
MEASURED on the MI355X, largest err_gpu / (err_cpu64 + floor / 8), every group within the margin 8:
                 Ghat   S     gamma  P     dxu   direct residual
  one row        1.6    2.0   1.7    3.4   3.3   4.4      (1..7 joints and the tree, N = 2, 3, 8, no soft limits)
  soft           1.9    1.6   1.8    2.5   2.9   4.2      (k_ginv_soft, both limit sets)
  wide           1.3    1.3   2.4    3.6   1.7   3.4      (arm8, arm12: k_ginv at 32 lanes per matrix)
  two rows       1.5    1.1   1.2    1.3   1.8   -        (arm7 N = 55, arm12 N = 33)
  GM forced      0.83   0.81  1.2    0.64  1.6   -        (arm3 N = 8, arm1 N = 2)
  GM natural     1.1    1.1   1.5    0.8   0.78  -        (arm6 N = 86)
A, Bm, c of the read-back are within 1e-12 of the oracle's on every group, arm12 included.  Hard limits: S_band
within 1.8e-14 and gamma within 1.2e-14 of the oracle's (bound 1e-10); 4..18 hard rows per problem; arm3's PCG
takes 43..100 iterations, arm6's runs to its cap of 100 on every problem (count and lambda still bit for bit).
The one-row and soft rows were measured again after the RNEA gradient's prismatic term was corrected:
tree4's A changed, and with it the tree's figures -- Ghat 1.2, S 1.2, gamma 1.7, P 2.2, dxu 3.3 (2.9 with soft
limits), direct 1.9; it now holds the dxu maximum of both rows and no longer the one-row gamma maximum.
No kernel was found wrong.
"""
import warnings

import numpy as np
import pytest

import qp_cases as qc
from ilqr_cases import box_limits
from oracle import canon, qp_hp
from oracle import sqp as osqp

pytestmark = pytest.mark.gpu

assert np.finfo(np.longdouble).eps < 2e-19, "long double is not an extended-precision format on this host"

DYN_TOL = 1e-12   # test_gpu_dynamics.py's, relative to max(1, max|ref|)


@pytest.fixture(scope="module")
def kctx():
    from trajoptmpcreference_amd import _native
    c = _native.Context(0)
    yield c
    c.set_reference(None)
    c.close()


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64 if a.dtype == np.float64 else a.dtype)


def _same(a, b):
    return np.array_equal(_bits(a), _bits(b))


def _run(ctx, g, method="PCG-SS", x=None, u=None, xs=None, rho=None, guess=None, soft=None):
    """one tmpc_qp_batch on the group's problems (or the given ones) and its read-back"""
    if x is None:
        x, u, xs = qc.problems(g.model, g.N, g.B, g.seed)
    if rho is None:
        rho = qc.rhos(g)
    m = qc.model(g.model)
    B = x.shape[0]
    ctx.set_model(m)
    ctx.set_cost_quadratic(*qc.cost_arrays(g.cost, m.n, g.N))
    ctx.set_options(precision=0)
    ctx.set_box_limits(box_limits(g.soft, m.n))
    if g.soft != "none":
        mu, lam = qc.soft_state(g) if soft is None else soft
        ctx.set_soft_state(B, g.N, mu=mu, lam=lam)   # right before the call (include/tmpc.h)
    q = ctx.qp_batch(x, u, g.N, qc.DT, rho, method, want_blocks=True, guess=guess, xs=xs)
    q.update(ctx.qp_last_inputs(B, g.N))
    nx = 2 * m.n
    q["lam"] = q["dxul"][:, -g.N * nx:]
    q["dxu"] = q["dxul"][:, :-g.N * nx]
    return q


def _close1(a, ref):
    return float(np.max(np.abs(np.asarray(a) - np.asarray(ref)))) / max(1.0, float(np.max(np.abs(ref))))


class Tally:
    """err_gpu / err_cpu64 per (group, rho, quantity): errors are the largest over the problems sharing a rho"""

    def __init__(self):
        self.e = {}

    def add(self, g, rho, what, e_gpu, e_cpu, floor=qc.FLOOR):
        k = (qc.gid(g), float(rho), what)
        a, b, _ = self.e.get(k, (0.0, 0.0, floor))
        self.e[k] = (max(a, e_gpu), max(b, e_cpu), floor)

    def check(self, title):
        bad, worst = [], {}
        for (gid, rho, what), (eg, ec, floor) in self.e.items():
            r = eg / (ec + floor / qc.MARGIN64) if ec + floor > 0 else (0.0 if eg == 0 else np.inf)
            worst[what] = max(worst.get(what, 0.0), r)
            print(f"{gid} rho={rho:g} {what}: err_gpu={eg:.3e} err_cpu64={ec:.3e} ratio={r:.3g}")
            if not eg <= qc.MARGIN64 * ec + floor:
                bad.append((gid, rho, what, f"err_gpu {eg:.3e}", f"err_cpu64 {ec:.3e}", f"ratio {r:.3g}"))
        warnings.warn(f"{title}: largest err_gpu / (err_cpu64 + floor / 8) per quantity "
                      + ", ".join(f"{k} {v:.2g}" for k, v in worst.items()))
        assert not bad, bad


def _parity(g, q, tally, dynamics=True, precond=True):
    """Ghat, S, gamma, P and the epilogue of one run against the long-double reference, into the tally"""
    nx = 2 * qc.model(g.model).n
    for b, rho in enumerate(qc.rhos(g)):
        if b not in qc.picked(g):   # Ghat alone: without soft limits the cost blocks are those of any problem
            assert g.soft == "none"   # with this rho
            r0 = next(b0 for b0 in qc.picked(g) if qc.rhos(g)[b0] == rho)
            Gxr, Gur = qc.blocks(qc.ghat_ref(g, r0), nx)
            Gx64, Gu64 = qc.blocks([np.linalg.inv(Gk + rho * np.eye(len(Gk))) for Gk in qc.kkt(g, r0)[0]], nx)
            tally.add(g, rho, "Ghat", max(qc.rel(q["Ghat_x"][b], Gxr), qc.rel(q["Ghat_u"][b], Gur)),
                      max(qc.rel(Gx64, Gxr), qc.rel(Gu64, Gur)))
            continue
        G, gg, Ao, Bo, co = qc.kkt(g, b)
        if dynamics:   # the read-back returns the right buffers
            e = [_close1(q["A"][b], Ao), _close1(q["Bm"][b], Bo), _close1(q["c"][b], co)]
            print(f"{qc.gid(g)} b={b}: A {e[0]:.2e} Bm {e[1]:.2e} c {e[2]:.2e} from the oracle's")
            assert max(e) <= DYN_TOL, (qc.gid(g), b, e)
        A, Bm, c = q["A"][b], q["Bm"][b], q["c"][b]
        Ghr = qc.ghat_ref(g, b)
        Gxr, Gur = qc.blocks(Ghr, nx)
        Gh64, Sd64, Sl64, gam64 = qc.cpu64_schur(g, b, A, Bm, c)
        Gx64, Gu64 = qc.blocks(Gh64, nx)
        tally.add(g, rho, "Ghat", max(qc.rel(q["Ghat_x"][b], Gxr), qc.rel(q["Ghat_u"][b], Gur)),
                  max(qc.rel(Gx64, Gxr), qc.rel(Gu64, Gur)))
        _, Sd, Sl, gam = qp_hp.schur_hp(G, gg, A, Bm, c, rho, nx, Gh=Ghr)
        tally.add(g, rho, "S", max(qc.rel(q["S_diag"][b], Sd), qc.rel(q["S_lo"][b], Sl)),
                  max(qc.rel(Sd64, Sd), qc.rel(Sl64, Sl)))
        tally.add(g, rho, "gamma", qc.rel(q["gamma"][b].reshape(g.N, nx), gam), qc.rel(gam64, gam))
        if precond:
            Pr = qp_hp.precond_diag_hp(q["S_diag"][b])
            tally.add(g, rho, "P", qc.rel(q["P_diag"][b], Pr), qc.rel(np.linalg.inv(q["S_diag"][b]), Pr))
        _epilogue(g, b, rho, q, tally, "dxu")


def _epilogue(g, b, rho, q, tally, name):
    """dxu of run q against dxu_hp with q's own lambda, Ghat from inv_hp, A and Bm from the read-back"""
    nx = 2 * qc.model(g.model).n
    G, gg = qc.kkt(g, b)[:2]
    A, Bm = q["A"][b], q["Bm"][b]
    ref = qp_hp.dxu_hp(qc.ghat_ref(g, b), gg, A, Bm, q["lam"][b], nx)
    Gh64 = [np.linalg.inv(Gk + rho * np.eye(len(Gk))) for Gk in G]
    c64 = osqp.recover_dxu(Gh64, gg, A, Bm, q["lam"][b], nx)[:ref.size]
    tally.add(g, rho, name, qc.rel(q["dxu"][b], ref), qc.rel(c64, ref))


def _direct(g, qs, tally):
    """method S's lambda: backward error on the GPU's own S, gamma against np.linalg.solve's"""
    nx = 2 * qc.model(g.model).n
    for b, rho in enumerate(qc.rhos(g)):
        if b not in qc.picked(g):
            continue
        Sd, Sl, gam = qs["S_diag"][b], qs["S_lo"][b], qs["gamma"][b]
        dense = osqp.dense_from_blocks(Sd, Sl, np.transpose(Sl, (0, 2, 1)))
        l64 = np.linalg.solve(dense, gam)
        eg, ec = qp_hp.backward_error(Sd, Sl, gam, qs["lam"][b]), qp_hp.backward_error(Sd, Sl, gam, l64)
        lr = qp_hp.solve_hp(Sd, Sl, gam).reshape(-1)
        print(f"{qc.gid(g)} b={b}: direct solve forward error gpu {qc.rel(qs['lam'][b], lr):.2e} "
              f"lapack {qc.rel(l64, lr):.2e} (cond {np.linalg.cond(dense):.1e})")
        tally.add(g, rho, "direct", eg, ec, floor=0.0)   # 8 x LAPACK's residual, no floor
        _epilogue(g, b, rho, qs, tally, "dxu-S")


# ------------------------------------------------------------------------------------------------ parity
def _part(key, part):
    """a model's groups in two parts: the horizon x cost x rho grid, and the rest (QF_start, the batches of 65
    and 1, the soft groups)"""
    gs = qc.groups_of(key)
    grid = [g for g in gs if g.soft == "none" and g.B == 8 and g.cost in ("default", "identity", "dense")]
    return grid if part == "grid" else [g for g in gs if g not in grid]


@pytest.mark.parametrize("part", ["grid", "rest"])
@pytest.mark.parametrize("key", qc.FULL_MODELS + qc.WIDE_MODELS)
def test_qp_kernels_against_extended_precision(kctx, key, part):
    """every group of the model: PCG-SS (Ghat, S, gamma, P, epilogue), then method S (the SCHUR-mode prologue
    gives the PCG run's bits; backward error of k_btsolve; the epilogue on its lambda) and method N (S's bits)"""
    tally = Tally()
    for g in _part(key, part):
        q = _run(kctx, g)
        _parity(g, q, tally)
        qs = _run(kctx, g, method="S")
        for f in ("A", "Bm", "c", "Ghat_x", "Ghat_u", "S_diag", "S_lo", "gamma"):
            assert _same(q[f], qs[f]), (qc.gid(g), f)
        assert np.all(qs["pcg_iters"] == 0)
        _direct(g, qs, tally)
        qn = _run(kctx, g, method="N")
        assert _same(qn["dxul"], qs["dxul"]), qc.gid(g)
    tally.check(f"QP kernels, {key} ({part})")


@pytest.mark.parametrize("key", ["arm3", "arm7", "arm12"])
def test_block_jacobi_preconditioner_blocks(kctx, key):
    """P_diag of PCG-BJ on the dense groups (PCG-SS: every group above)"""
    tally = Tally()
    nx = 2 * qc.model(key).n
    for g in [g for g in qc.groups_of(key) if g.cost in qc.DENSE and g.B == 8]:
        q = _run(kctx, g, method="PCG-BJ")
        for b, rho in enumerate(qc.rhos(g)):
            Pr = qp_hp.precond_diag_hp(q["S_diag"][b])
            tally.add(g, rho, "P", qc.rel(q["P_diag"][b], Pr), qc.rel(np.linalg.inv(q["S_diag"][b]), Pr))
            _epilogue(g, b, rho, q, tally, "dxu")
    assert nx and tally.e
    tally.check(f"PCG-BJ preconditioner blocks, {key}")


@pytest.mark.parametrize("name", list(qc.INSTANCES))
def test_qp_instances_against_extended_precision(kctx, name, monkeypatch):
    """the fused kernel's instances (one row per lane, two rows in registers, the HBM-row GM instance forced and
    past its natural threshold): parity, and count and lambda bit for bit the canonical-order PCG's"""
    g, gm = qc.INSTANCES[name]
    if gm is None:
        monkeypatch.delenv("TMPC_QP_GM_MIN_ROWS", raising=False)
    else:
        monkeypatch.setenv("TMPC_QP_GM_MIN_ROWS", str(gm))
    nx = 2 * qc.model(g.model).n
    tally = Tally()
    q = _run(kctx, g)
    _parity(g, q, tally)
    _replay(g, q, "SS", canon.qp_rpl(g.N, nx, gm))
    tally.check(f"QP instance {name}")


# ------------------------------------------------------------------------------------------------ PCG replay
def _replay(g, q, pre, rpl, guess=None, o=None):
    """count and lambda of run q are oracle/canon.c's on q's own S, gamma"""
    o = osqp.default_options(o)
    for b in range(q["lam"].shape[0]):
        lam, it, _ = canon.pcg(q["S_diag"][b], q["S_lo"][b], q["gamma"][b], pre, tol=o["exit_tolerance_linSys"],
                               max_iter=o["max_iter_linSys"], rpl=rpl, guess=None if guess is None else guess[b])
        assert it == int(q["pcg_iters"][b]), (qc.gid(g), pre, b, it, int(q["pcg_iters"][b]))
        print(f"{qc.gid(g)} PCG-{pre} b={b}: {it} iterations{' (warm)' if guess is not None else ''}")
        assert _same(lam, q["lam"][b]), (qc.gid(g), pre, b)


PCG_GROUPS = [qc.Group("arm3", 8, "dense", "none", 8, 600, "mixed"), qc.Group("arm6", 8, "qfstart-dense", "none", 8, 621, "mixed"),
              qc.Group("arm7", 8, "dense", "joint+torque", 8, 680, "mixed"), qc.Group("arm12", 8, "dense", "none", 8, 600, "mixed")]


@pytest.mark.parametrize("pre", ["J", "BJ", "SS", "0"])
@pytest.mark.parametrize("g", PCG_GROUPS, ids=qc.gid)
def test_pcg_is_bitwise_the_canonical_order_on_dense_costs(kctx, g, pre, monkeypatch):
    """B = 8 with mixed rho; cold, and warm-started from a perturbed lambda.  The epilogue on the PCG's own lambda
    is held to dxu_hp, apart from how well the PCG converged"""
    monkeypatch.delenv("TMPC_QP_GM_MIN_ROWS", raising=False)
    nx = 2 * qc.model(g.model).n
    rpl = canon.qp_rpl(g.N, nx)
    tally = Tally()
    q = _run(kctx, g, method=f"PCG-{pre}")
    _replay(g, q, pre, rpl)
    guess = q["lam"] * (1 + 1e-3 * np.random.default_rng(5).standard_normal(q["lam"].shape))
    w = _run(kctx, g, method=f"PCG-{pre}", guess=guess)
    _replay(g, w, pre, rpl, guess=guess)
    assert not _same(w["lam"], q["lam"]), (qc.gid(g), pre, "the guess was not used")
    for r in (q, w):
        for b, rho in enumerate(qc.rhos(g)):
            _epilogue(g, b, rho, r, tally, "dxu")
    tally.check(f"epilogue after PCG-{pre}, {qc.gid(g)}")


@pytest.mark.parametrize("name", ["two-rows-arm7", "gm-forced-arm3", "gm-natural"])
def test_pcg_warm_start_in_the_two_row_layouts(kctx, name, monkeypatch):
    g, gm = qc.INSTANCES[name]
    if gm is None:
        monkeypatch.delenv("TMPC_QP_GM_MIN_ROWS", raising=False)
    else:
        monkeypatch.setenv("TMPC_QP_GM_MIN_ROWS", str(gm))
    nx = 2 * qc.model(g.model).n
    q = _run(kctx, g, method="PCG-BJ")
    _replay(g, q, "BJ", canon.qp_rpl(g.N, nx, gm))
    guess = q["lam"] * (1 + 1e-3 * np.random.default_rng(6).standard_normal(q["lam"].shape))
    w = _run(kctx, g, method="PCG-BJ", guess=guess)
    _replay(g, w, "BJ", canon.qp_rpl(g.N, nx, gm), guess=guess)


# ------------------------------------------------------------------------------------------------ exact relations
FIELDS = ("A", "Bm", "c", "Ghat_x", "Ghat_u", "S_diag", "S_lo", "gamma", "P_diag", "dxul", "pcg_iters")


@pytest.mark.parametrize("method", ["PCG-SS", "S"])
@pytest.mark.parametrize("key", ["arm3", "arm6", "arm12"])
def test_a_problem_does_not_depend_on_its_batch(kctx, key, method):
    """problem p alone equals, bit for bit, itself at positions 0, 31 and 64 of a batch of 65 with mixed rho (195
    Ghat matrices, four or two to a wave: its wave holds other problems' matrices at other rho)"""
    g = next(g for g in qc.groups_of(key) if g.B == 65)
    x, u, xs = qc.problems(g.model, g.N, g.B, g.seed)
    xp, up, sp = (a[1:] for a in qc.problems(g.model, g.N, 2, 800))
    rp = np.array([1.0])
    alone = _run(kctx, g, method=method, x=xp, u=up, xs=sp, rho=rp)
    for pos in (0, 31, 64):
        xb, ub, sb, rb = x.copy(), u.copy(), xs.copy(), qc.rhos(g)
        xb[pos], ub[pos], sb[pos], rb[pos] = xp[0], up[0], sp[0], rp[0]
        r = _run(kctx, g, method=method, x=xb, u=ub, xs=sb, rho=rb)
        for f in FIELDS:
            if f != "P_diag" or method != "S":
                assert _same(r[f][pos], alone[f][0]), (key, method, pos, f)


@pytest.mark.parametrize("g", [qc.INSTANCES["one-row"][0], qc.Group("arm6", 8, "qfstart-dense", "none", 8, 621, "mixed"),
                               qc.Group("arm5", 8, "dense", "joint+torque", 8, 680, "mixed")], ids=qc.gid)
def test_schur_blocks_are_the_same_bits_in_every_instance(kctx, g, monkeypatch):
    """the one-row instance, the forced GM instance and method S's SCHUR-mode prologue all call qp_schur_row"""
    monkeypatch.delenv("TMPC_QP_GM_MIN_ROWS", raising=False)
    one = _run(kctx, g)
    s = _run(kctx, g, method="S")
    monkeypatch.setenv("TMPC_QP_GM_MIN_ROWS", "1")
    gm = _run(kctx, g)
    for f in ("A", "Bm", "c", "Ghat_x", "Ghat_u", "S_diag", "S_lo", "gamma"):
        assert _same(one[f], s[f]) and _same(one[f], gm[f]), (qc.gid(g), f)
    assert _same(one["P_diag"], gm["P_diag"])


@pytest.mark.parametrize("method", ["PCG-SS", "S"])
def test_diagonal_blocks_take_the_generic_path_bits(kctx, method, monkeypatch):
    """dense arrays whose blocks happen to be diagonal (distinct entries, a goal): CostDev.diag's fast path gives
    TMPC_GENERIC_COST=1's bits in every output of the QP"""
    key, N, B = "arm6", 8, 8
    m = qc.model(key)
    rng = np.random.default_rng(77)
    Q, QF, R = (np.diag(rng.uniform(0.5, 2.0, k)) for k in (2 * m.n, 2 * m.n, m.n))
    xg = rng.uniform(-0.5, 0.5, 2 * m.n)
    x, u, xs = qc.problems(key, N, B, 600)
    out = []
    for generic in ("0", "1"):
        monkeypatch.setenv("TMPC_GENERIC_COST", generic)
        kctx.set_model(m)
        kctx.set_cost_quadratic(Q, QF, R, xg, N // 2)   # the variable is read here
        kctx.set_options(precision=0)
        kctx.set_box_limits(None)
        q = kctx.qp_batch(x, u, N, qc.DT, qc.cases.mixed_rhos(B), method, xs=xs)
        q.update(kctx.qp_last_inputs(B, N))
        out.append(q)
    for f in FIELDS:
        if f != "P_diag" or method != "S":
            assert _same(out[0][f], out[1][f]), (method, f)
    assert np.max(np.abs(out[0]["dxul"])) > 0


@pytest.mark.parametrize("method", ["PCG-SS", "S"])
@pytest.mark.parametrize("key", ["arm3", "arm7"])
def test_a_constant_reference_equal_to_the_goal_is_the_fixed_goal(kctx, key, method):
    """tmpc_set_reference with xref = xg at every knot, on a dense cost: the tracking instance's bits are the
    fixed-goal instance's"""
    g = qc.Group(key, 8, "qfstart-dense", "none", 8, 621, "mixed")
    xg = qc.cost_arrays(g.cost, qc.model(key).n, g.N)[3]
    assert np.max(np.abs(xg)) > 0
    kctx.set_reference(None)
    fixed = _run(kctx, g, method=method)
    try:
        kctx.set_model(qc.model(key))
        kctx.set_reference(np.repeat(xg[None, :, None], g.N, axis=2))
        track = _run(kctx, g, method=method)
    finally:
        kctx.set_reference(None)
    for f in FIELDS:
        if f != "P_diag" or method != "S":
            assert _same(fixed[f], track[f]), (key, method, f)


# ------------------------------------------------------------------------------------------------ hard limits
def _hard_problems(key, N, B, seed):
    """qp_cases' problems pushed over the +-2.0 limits: the planar arms' rollouts of u = 0 stand still, so the
    velocities take U(-2.3, 2.3) and the controls are scaled to U(-2.3, 2.3): about one row in eight is active
    (a third of the rows active leaves more rows than variables: S singular, every PCG at its cap)"""
    x, u, xs = qc.problems(key, N, B, seed)
    n = u.shape[1]
    rng = np.random.default_rng(seed + 31)
    x = x.copy()
    x[:, n:, :] += rng.uniform(-2.3, 2.3, x[:, n:, :].shape)
    return x, 11.5 * u, xs


@pytest.mark.parametrize("method", ["PCG-SS", "PCG-BJ"])
@pytest.mark.parametrize("key", ["arm3", "arm6"])
def test_hard_limit_qp_on_a_dense_cost(kctx, key, method):
    """ACTIVE_SET torque + velocity limits at +-2.0, dense Q, QF, R and a goal, B = 4 with mixed rho: the banded
    kernels on full Ghat blocks.  Active sets and dimension are oracle/hard.py's; S_band and gamma at
    test_gpu_hard.py's 1e-10; pcg_canonical on the GPU's own band gives the GPU's count and lambda bit for bit"""
    from oracle import hard as ohard
    from test_gpu_hard import _row_layout, _unband
    N, B = 8, 4
    g = qc.Group(key, N, "dense", "none", B, 900, "mixed")
    m = qc.model(key)
    n, nx = m.n, 2 * m.n
    x, u, xs = _hard_problems(key, N, B, g.seed)
    hard = ohard.HardConstraints([ohard.HardLimit(k, n, -2.0, 2.0, "ACTIVE_SET") for k in ("velocity", "torque")])
    cost, rho = qc.quad_cost(g), qc.rhos(g)
    kctx.set_model(m)
    kctx.set_cost_quadratic(*qc.cost_arrays(g.cost, n, N))
    kctx.set_options(precision=0)
    kctx.set_box_limits({k: dict(mode="ACTIVE_SET", lb=[-2.0] * n, ub=[2.0] * n) for k in ("velocity", "torque")})
    try:
        q = kctx.qp_batch(x, u, N, qc.DT, rho, method, want_blocks=False, xs=xs)
        info = kctx.qp_hard_info(B, N)
    finally:
        kctx.set_box_limits(None)
    o = osqp.default_options()
    nz = (nx + n) * (N - 1) + nx
    for b in range(B):
        masks = hard.active_masks(x[b], u[b], N)
        assert sum(v != 0 for v in masks) >= 2, (key, b, "fewer than two knots with an active row")
        assert [int(v) for v in info["active"][b]] == masks, (key, b)
        G, gg, Cm, cc = ohard.kkt_dense(m, cost, x[b], u[b], xs[b], N, qc.DT, hard)
        D = Cm.shape[0]
        assert nx * N < D == int(info["dim"][b]), (key, b)
        invG = np.linalg.inv(G + rho[b] * np.eye(G.shape[0]))
        S_o, gam_o = -Cm @ (invG @ Cm.T), cc - Cm @ (invG @ gg)
        S_g, gam_g = _unband(info["S_band"][b], info["W"], D), info["gamma"][b, :D]
        eS = float(np.max(np.abs(S_g - S_o))) / float(np.max(np.abs(S_o)))
        eg = float(np.max(np.abs(gam_g - gam_o))) / max(1.0, float(np.max(np.abs(gam_o))))
        lam_c, it_c = ohard.pcg_canonical(S_g, gam_g, nx, method[4:], o["exit_tolerance_linSys"], o["max_iter_linSys"])
        print(f"{key} {method} b={b} rho={rho[b]:g}: {D - nx * N} hard rows, S {eS:.2e} gamma {eg:.2e}, "
              f"{int(q['pcg_iters'][b])} PCG iterations")
        assert eS <= 1e-10 and eg <= 1e-10, (key, b, eS, eg)
        assert int(q["pcg_iters"][b]) == it_c, (key, b, int(q["pcg_iters"][b]), it_c)
        dyn, hrows = _row_layout(hard, x[b], u[b], N, nx)
        assert np.array_equal(q["dxul"][b][nz:], lam_c[dyn]), (key, b)
        lam_hard = np.array([info["lambda_hard"][b, k, sl] for _, k, sl in hrows])
        assert np.array_equal(lam_hard, lam_c[[a for a, _, _ in hrows]]), (key, b)


# ------------------------------------------------------------------------------------------------ the read-back
def test_read_back_refuses_what_it_cannot_report(kctx):
    from trajoptmpcreference_amd import _native
    g = qc.Group("arm3", 8, "dense", "none", 2, 600, 1.0)
    _run(kctx, g)
    with pytest.raises(_native.NativeError, match="B=2 N=8"):
        kctx.qp_last_inputs(3, 8)
    with pytest.raises(_native.NativeError, match="B=2 N=8"):
        kctx.qp_last_inputs(2, 7)
    assert kctx.lib.tmpc_qp_last_inputs(kctx.h, 2, 8, None, None, None, None, None) == 0   # every output nullable
    # another user of the buffers: the record is cleared
    x, u, _ = qc.problems(g.model, g.N, g.B, g.seed)
    kctx.sqp_solve_batch(x.copy(), u.copy(), g.N, qc.DT, "PCG-SS")
    with pytest.raises(_native.NativeError, match="no tmpc_qp_batch call"):
        kctx.qp_last_inputs(2, 8)
    # the banded path
    kctx.set_box_limits({"torque": dict(mode="ACTIVE_SET", lb=[-2.0] * 3, ub=[2.0] * 3)})
    try:
        xs = qc.problems(g.model, g.N, g.B, g.seed)[2]
        kctx.qp_batch(x, u, g.N, qc.DT, 1.0, "PCG-SS", want_blocks=False, xs=xs)
        with pytest.raises(_native.NativeError, match="banded path"):
            kctx.qp_last_inputs(2, 8)
    finally:
        kctx.set_box_limits(None)
    # a fresh context has nothing to report
    c = _native.Context(0)
    try:
        c.set_model(qc.model("arm3"))
        with pytest.raises(_native.NativeError, match="no tmpc_qp_batch call"):
            c.qp_last_inputs(2, 8)
    finally:
        c.close()
