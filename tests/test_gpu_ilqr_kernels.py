"""Unit parity of the iLQR kernels (k_ilqr_backward, k_ilqr_forward, k_ilqr_soft_add) through
tmpc_ilqr_step_batch, which returns one iteration's own outputs: the integrator Jacobians the sweep consumed,
K, d, (dV1, dV2), ok, and every line-search trial's rollout and cost.  Inputs: tests/ilqr_cases.py (their
conditioning is checked on the CPU by test_oracle_ilqr_hp.py).

Backward sweep.  The reference is oracle/ilqr.py backward_hp in long double on the GPU's own A, B (which
isolates the sweep from the dynamics gradient; that is compared with rbd.euler_gradient at
test_gpu_dynamics.py's 1e-12 once per model).  Per (group, rho) and for each of K, d, dV, with
err = max|a - ref| / max(1, max|ref|) over the group's problems:
  fp64:  err_gpu <= 8 err_cpu64 + 1e-14, err_cpu64 the canonical-order CPU sweep (oilqr.backward) -- the kernel
         sums the same products in another order with fused multiply-adds, so its error is of the CPU
         restatement's size; a structural error is seven or more orders above it;
  fp32:  err_gpu <= 4 err_cpu32, err_cpu32 a plain float32 sweep (backward_hp with dtype = float32), both
         TMPC_ILQR_F32_VALU settings, and the result differs from the fp64 run's.
A (group, rho) of these tests has at least 8 problems (tests/ilqr_cases.py says why).
MEASURED on the MI355X (the tests print every figure and raise each case's largest ratio as a warning), largest
err_gpu / err_cpu per model, every group within its margin:
  fp64 (margin 8):  arm1 0.88, arm2 1.4, arm3 4.2, arm4 1.9, arm5 2.7, arm6 4.4, arm7 3.5, tree4 1.3, arm8 3.1,
                    arm12 2.0;
  fp32 matrix-core (margin 4):  arm3 2.9, arm6 3.0, arm7 3.4;   fp32 VALU (margin 4):  arm3 2.8, arm6 2.9, arm7 2.4.
Every sample of a group is informative (cases.sweep_errors asserts d != 0, dV != 0).  A first layout kept u = 0 for
the even problems at N = 2 too, where d = 0 and dV = 0 exactly (tests/ilqr_cases.py): those groups then had 4
samples that compared 0 with 0 and 4 with |d|, |dV| < 0.1, and the fp32 ratios of four N = 2 cases came out at
4.0 .. 7.85 on errors of 1e-9 .. 3e-8 -- one or two rounding draws against each other, per problem 0.3 .. 5 fp32
units in the last place of the entry (up to 88 where Q_u = l_u + B^T V_x cancels, on the CPU sweep's side up to 24).

Exact relations (bitwise, no tolerance): the matrix-core sweep against TMPC_ILQR_VALU=1 (the same
products in the same order), the prefetching rollout against TMPC_ILQR_NOPF=1 at T = 9, 2 and 1 trials, a
problem alone against the same problem at positions 0, 31 and 64 of a batch of 65, and a batch with one
failed factorisation (rho = -1e3) against the batch without that problem.

Forward sweep.  With the GPU's own K, d every trial's xt, ut against oilqr.forward and Jt against
osqp.total_cost, relative to max(1, max|ref|); trials with max|x| > 1e3 are left out (at most a quarter of a
group's; measured: at most 11 of 72), and a trial the oracle finds non-finite must be non-finite on the GPU.  The
bounds are 8 x the largest deviation measured on the MI355X, under the ceilings 1e-9 (fp64 rollouts: precision 0
and 1) and 1e-4 (fp32 rollouts: precision 2):
  fp64 rollouts   measured 2.71e-12 (arm6 N = 16; precision 1: 1.19e-12)  -> bound 2.2e-11;
  fp32 rollouts   measured 4.42e-05 (arm7 N = 8, B = 65; arm6 9.9e-06, arm3 5.3e-07, tree4 2.8e-07); 8 x that is
                  3.5e-04, past the ceiling, so the bound is the ceiling 1e-4 (2.3 x the measured value).
A wrong knot's gain (K[k+1] used at knot k in the comparison) deviates by 3.8e-01 (arm6) and 4.8e-01 (arm7).
tree4's figures are those measured after the RNEA gradient's prismatic term was corrected, which
changed its A: 1.3 was 1.5, 2.8e-07 was 3.1e-07; its fp64 rollouts deviate by at most 3.6e-15.
"""
import warnings

import numpy as np
import pytest

import ilqr_cases as cases
from oracle import ilqr as oilqr
from oracle import sqp as osqp

pytestmark = pytest.mark.gpu

assert np.finfo(np.longdouble).eps < 2e-19, "long double is not an extended-precision format on this host"

MARGIN64, MARGIN32 = 8.0, 4.0
# largest deviation of a trial from oilqr.forward / osqp.total_cost measured on the MI355X, by rollout precision,
# and the bound: 8 x the measured value, at most the ceiling
FWD_MEASURED = {"fp64": 2.71e-12, "fp32": 4.42e-05}
FWD_CEILING = {"fp64": 1e-9, "fp32": 1e-4}
FWD_BOUND = {k: min(8 * FWD_MEASURED[k], FWD_CEILING[k]) for k in FWD_MEASURED}
assert FWD_BOUND["fp64"] <= 1e-9 and FWD_BOUND["fp32"] <= 1e-4

OUTPUTS = ("A", "Bm", "K", "d", "dV", "ok", "alphas", "xt", "ut", "Jt")
SWEEP = ("K", "d", "dV", "ok")
TRIALS = ("xt", "ut", "Jt")


@pytest.fixture(scope="module")
def kctx():
    from trajoptmpcreference_amd import _native
    c = _native.Context(0)
    yield c
    c.close()


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64 if a.dtype == np.float64 else a.dtype)


def _same(a, b):
    """bit for bit (np.array_equal on the bit patterns: a diverged trial's NaNs compare too)"""
    return np.array_equal(_bits(a), _bits(b))


def _configure(ctx, g, B, precision=0, alpha_min=0.005):
    m = cases.model(g.model)
    ctx.set_model(m)
    ctx.set_cost_quadratic(*cases.cost_arrays(g.cost, m.n, g.N))
    ctx.set_options(precision=precision, alpha_min_SQP_DDP=alpha_min, alpha_factor_SQP_DDP=0.5)
    ctx.set_box_limits(cases.box_limits(g.soft, m.n))
    if g.soft != "none":
        ctx.set_soft_state(B, g.N)   # the limits' initial constants


def _run(ctx, g, trials=True, precision=0, alpha_min=0.005, x=None, u=None, rho=None):
    if x is None:
        x, u = cases.problems(g.model, g.N, g.B, g.seed)
    if rho is None:
        rho = cases.rhos(g)
    _configure(ctx, g, x.shape[0], precision, alpha_min)
    return ctx.ilqr_step_batch(x, u, g.N, cases.DT, rho, want_trials=trials)


def _gpu_sweep(r):
    return lambda b, A, Bm, dv, rho: (r["K"][b], r["d"][b], r["dV"][b, 0], r["dV"][b, 1])


def _check_ratio(g, errs, cand, base, margin, slack, worst, bad):
    """prints every figure; what misses err_cand <= margin err_base + slack goes to `bad` (asserted empty by the
    test once all its groups are printed)"""
    for rho, e in errs.items():
        for what in ("K", "d", "dV"):
            eg, ec = e[cand][what], e[base][what]
            ratio = eg / (ec + slack / margin) if ec + slack > 0 else (0.0 if eg == 0 else np.inf)
            worst[cases.gid(g)] = max(worst.get(cases.gid(g), 0.0), ratio)
            print(f"{cases.gid(g)} rho={rho:g} {what}: err_{cand}={eg:.3e} err_{base}={ec:.3e} ratio={ratio:.3g}")
            if not eg <= margin * ec + slack:
                bad.append((cases.gid(g), rho, what, f"err_{cand} {eg:.3e}", f"err_{base} {ec:.3e}", f"ratio {ratio:.3g}"))


def _report(title, worst):
    top = max(worst.values()) if worst else 0.0
    warnings.warn(f"{title}: largest err_gpu / err_cpu = {top:.3g}; per group "
                  + ", ".join(f"{k} {v:.2g}" for k, v in worst.items()))


# ------------------------------------------------------------------------------------------------ backward
@pytest.mark.parametrize("key", cases.FULL_MODELS + cases.WIDE_MODELS)
def test_backward_fp64_against_extended_precision(kctx, key):
    worst, bad = {}, []
    for g in cases.groups_of(key):
        r = _run(kctx, g, trials=False)
        # for the record, once per horizon: the Jacobians (the wide models' are pinned by test_gpu_wide.py on
        # its own states; at arm12's N = 8 states here they are 2.9e-12 from the oracle's)
        if key in cases.FULL_MODELS and g.cost == "default" and g.soft == "none":
            Ar, Br = cases.cpu_jacobians(g)
            assert cases.rel_err(r["A"], Ar) <= 1e-12 and cases.rel_err(r["Bm"], Br) <= 1e-12, cases.gid(g)
        errs = cases.sweep_errors(g, r["A"], r["Bm"], {"gpu": _gpu_sweep(r), "cpu64": cases.cpu64_sweep}, ok=r["ok"])
        _check_ratio(g, errs, "gpu", "cpu64", MARGIN64, 1e-14, worst, bad)
    _report(f"fp64 backward sweep, {key}", worst)
    assert not bad, bad


@pytest.mark.parametrize("N", [2, 3, 8], ids=["N2", "N3", "N8"])
@pytest.mark.parametrize("valu", [False, True], ids=["mfma", "valu"])
@pytest.mark.parametrize("key", cases.F32_MODELS)
def test_backward_fp32_against_extended_precision(kctx, key, valu, N, monkeypatch):
    """precision = 1: both fp32 instances of the sweep against a plain float32 sweep's error"""
    if valu:
        monkeypatch.setenv("TMPC_ILQR_F32_VALU", "1")
    else:
        monkeypatch.delenv("TMPC_ILQR_F32_VALU", raising=False)
    monkeypatch.delenv("TMPC_ILQR_VALU", raising=False)
    worst, bad = {}, []
    for g in [g for g in cases.f32_groups_of(key) if g.N == N]:
        r = _run(kctx, g, trials=False, precision=1)
        errs = cases.sweep_errors(g, r["A"], r["Bm"], {"gpu": _gpu_sweep(r), "cpu32": cases.cpu32_sweep}, ok=r["ok"])
        _check_ratio(g, errs, "gpu", "cpu32", MARGIN32, 0.0, worst, bad)
        r64 = _run(kctx, g, trials=False, precision=0)
        assert not np.array_equal(r["K"], r64["K"]) and not np.array_equal(r["d"], r64["d"]), cases.gid(g)
    _report(f"fp32 backward sweep ({'VALU' if valu else 'matrix-core'}), {key} N = {N}", worst)
    assert not bad, bad


def test_fp32_sweep_instances_differ(kctx, monkeypatch):
    """TMPC_ILQR_F32_VALU is read at each launch: the two fp32 instances round differently somewhere"""
    g = cases.Group("arm6", 8, "dense", "none", 8, 500, "mixed")
    monkeypatch.delenv("TMPC_ILQR_F32_VALU", raising=False)
    a = _run(kctx, g, trials=False, precision=1)
    monkeypatch.setenv("TMPC_ILQR_F32_VALU", "1")
    b = _run(kctx, g, trials=False, precision=1)
    assert _same(a["A"], b["A"]) and _same(a["Bm"], b["Bm"])
    assert not _same(a["K"], b["K"])


# ------------------------------------------------------------------------------------------------ exact relations
@pytest.mark.parametrize("key", cases.FULL_MODELS)
def test_matrix_core_sweep_is_bitwise_the_valu_sweep(kctx, key, monkeypatch):
    """every output of the fp64 matrix-core sweep is the same products summed in the same order as the
    VALU loops' -- 1..7 joints (and the tree), soft limits on and off, every horizon and cost of the groups"""
    for g in cases.groups_of(key):
        rho = cases.mixed_rhos(g.B)   # different values inside every batch
        monkeypatch.delenv("TMPC_ILQR_VALU", raising=False)
        a = _run(kctx, g, trials=False, rho=rho)
        monkeypatch.setenv("TMPC_ILQR_VALU", "1")
        b = _run(kctx, g, trials=False, rho=rho)
        assert np.all(a["ok"] == 1), cases.gid(g)
        for f in SWEEP:
            assert _same(a[f], b[f]), (cases.gid(g), f, float(np.max(np.abs(a[f] - b[f]))))


@pytest.mark.parametrize("alpha_min,T", [(0.005, 9), (0.6, 2), (1.0, 1)])
@pytest.mark.parametrize("key", cases.FULL_MODELS)
def test_prefetching_rollout_is_bitwise_the_plain_rollout(kctx, key, alpha_min, T, monkeypatch):
    """prefetching moves data only: TMPC_ILQR_NOPF=1 (the plain instance) gives the same trials bit for bit"""
    for g in cases.groups_of(key):
        rho = cases.mixed_rhos(g.B)   # different values inside every batch
        monkeypatch.delenv("TMPC_ILQR_NOPF", raising=False)
        a = _run(kctx, g, alpha_min=alpha_min, rho=rho)
        monkeypatch.setenv("TMPC_ILQR_NOPF", "1")
        b = _run(kctx, g, alpha_min=alpha_min, rho=rho)
        assert a["xt"].shape[1] == T and list(a["alphas"]) == [0.5 ** t for t in range(T)], cases.gid(g)
        for f in SWEEP + TRIALS:
            assert _same(a[f], b[f]), (cases.gid(g), f)


@pytest.mark.parametrize("soft", ["none", "joint+torque"])
@pytest.mark.parametrize("key", ["arm3", "arm5", "arm7", "tree4"])
def test_a_problem_does_not_depend_on_its_batch(kctx, key, soft):
    """problem p alone equals, bit for bit and in every output, its rows at positions 0, 31 and 64 of a batch of
    65 other problems (lane and group indexing at the 64-lane group boundaries)"""
    g = cases.Group(key, 8, "dense", soft, 65, 540, "mixed")
    x, u = cases.problems(g.model, g.N, g.B, g.seed)
    xp, up = cases.problems(g.model, g.N, 2, 700)
    xp, up, rp = xp[1:], up[1:], np.array([1.0])
    alone = _run(kctx, g, x=xp, u=up, rho=rp)
    assert int(alone["ok"][0]) == 1 and np.any(np.isfinite(alone["Jt"][0]))
    for pos in (0, 31, 64):
        xb, ub, rb = x.copy(), u.copy(), cases.rhos(g)
        xb[pos], ub[pos], rb[pos] = xp[0], up[0], rp[0]
        r = _run(kctx, g, x=xb, u=ub, rho=rb)
        for f in OUTPUTS:
            if f != "alphas":
                assert _same(r[f][pos], alone[f][0]), (key, soft, pos, f)
        assert _same(r["alphas"], alone["alphas"])


@pytest.mark.parametrize("key", ["arm3", "arm6", "arm7"])
def test_a_failed_factorisation_stays_local(kctx, key):
    """one problem with rho = -1e3 (Q_uu not positive definite: ok = 0, the reference returns None): the other
    problems' outputs are those of the batch without it, bit for bit"""
    g = cases.Group(key, 8, "identity", "none", 8, 500, "mixed")
    x, u = cases.problems(g.model, g.N, g.B, g.seed)
    bad = 3
    rho = cases.rhos(g)
    rho[bad] = -1e3
    r = _run(kctx, g, x=x, u=u, rho=rho)
    assert oilqr.backward_hp(r["A"][bad], r["Bm"][bad], *cases.derivatives(g, bad), rho[bad]) is None
    keep = [b for b in range(g.B) if b != bad]
    assert int(r["ok"][bad]) == 0 and np.all(r["ok"][keep] == 1)
    w = _run(kctx, g, x=x[keep], u=u[keep], rho=rho[keep])
    for f in OUTPUTS:
        if f != "alphas":
            assert _same(r[f][keep], w[f]), (key, f)


def test_step_refuses_what_the_solve_refuses(kctx):
    from trajoptmpcreference_amd import _native
    g = cases.Group("arm3", 8, "default", "none", 2, 500, 1.0)
    x, u = cases.problems(g.model, g.N, g.B, g.seed)
    _configure(kctx, g, g.B)
    lib, out = kctx.lib, kctx.ilqr_step_batch(x, u, g.N, cases.DT, 1.0)
    assert out["xt"].shape == (2, 9, 6, 8)
    # the caller's T must be the options' schedule
    rho = np.ones(2)
    rc = lib.tmpc_ilqr_step_batch(kctx.h, 2, 8, 0.1, _native._ptr(np.ascontiguousarray(x)),
                                  _native._ptr(np.ascontiguousarray(u)), _native._ptr(rho), 8, *([None] * 10))
    assert rc != 0 and b"T = 8" in lib.tmpc_last_error(kctx.h)
    # a null context is an error, not a crash
    assert lib.tmpc_ilqr_step_batch(None, 2, 8, 0.1, None, None, None, 9, *([None] * 10)) < 0
    # UrdfCost
    m2 = cases.model("arm2")
    x2, u2 = cases.problems("arm2", 8, 2, 500)
    kctx.set_model(m2)
    kctx.set_cost_ee(np.eye(4), np.eye(4), np.eye(2), np.zeros(4), None, m2.H0[:2], m2.Ha[:2], m2.Hb[:2])
    with pytest.raises(_native.NativeError, match="QuadraticCost only"):
        kctx.ilqr_step_batch(x2, u2, 8, cases.DT, 1.0)
    _configure(kctx, g, g.B)
    kctx.set_box_limits({"torque": dict(mode="ACTIVE_SET", lb=[-1.0] * 3, ub=[1.0] * 3)})
    with pytest.raises(_native.NativeError, match="hard box constraints"):
        kctx.ilqr_step_batch(x, u, g.N, cases.DT, 1.0)
    kctx.set_box_limits(None)
    wide = cases.Group("arm8", 8, "default", "none", 2, 500, 1.0)
    xw, uw = cases.problems(wide.model, wide.N, wide.B, wide.seed)
    _configure(kctx, wide, wide.B)
    kctx.set_options(precision=1)
    with pytest.raises(_native.NativeError, match="fp64 only"):
        kctx.ilqr_step_batch(xw, uw, wide.N, cases.DT, 1.0)
    kctx.set_options(precision=0)


# ------------------------------------------------------------------------------------------------ forward
def _forward_groups(key):
    """every horizon, cost branch (diagonal / dense / QF_start), soft-limit set and batch size of the model's
    groups once (the wide models: two groups, their oracle rollouts are the slowest)"""
    if key in cases.WIDE_MODELS:
        return [cases.Group(key, 2, "default", "none", 8, 500, 1e-3), cases.Group(key, 8, "dense", "none", 8, 500, 1.0)]
    return [g for g in cases.groups_of(key)
            if g.soft != "none" or g.B != 8 or (g.N, g.cost) in ((2, "default"), (3, "dense"), (8, "dense"),
                                                                 (8, "qfstart"), (16, "default"))]


def _check_forward(ctx, g, precision, kind, worst):
    r = _run(ctx, g, precision=precision)
    m = cases.model(g.model)
    x, u = cases.problems(g.model, g.N, g.B, g.seed)
    cost = cases.quad_cost(g)
    soft = cases.soft_oracle(g.soft, m.n, g.N)
    T = len(r["alphas"])
    assert list(r["alphas"]) == [0.5 ** t for t in range(T)]
    assert np.all(r["ok"] == 1), cases.gid(g)
    picked = range(g.B) if g.B <= 8 else (0, 1, 31, 32, 63, 64)   # both sides of the 64-lane group boundaries
    left_out = total = 0
    dev = 0.0
    for b in picked:
        for t in range(T):
            total += 1
            with np.errstate(all="ignore"):
                xn, un = oilqr.forward(m, x[b], u[b], r["K"][b], r["d"][b], r["alphas"][t], cases.DT)
                Jn = osqp.total_cost(cost, xn, un, g.N, soft)
            if not (np.all(np.isfinite(xn)) and np.all(np.isfinite(un)) and np.isfinite(Jn)):
                assert not (np.all(np.isfinite(r["xt"][b, t])) and np.isfinite(r["Jt"][b, t])), (cases.gid(g), b, t)
                left_out += 1
                continue
            if np.max(np.abs(xn)) > 1e3:
                left_out += 1
                continue
            e = max(cases.rel_err(r["xt"][b, t], xn), cases.rel_err(r["ut"][b, t], un),
                    cases.rel_err(r["Jt"][b, t], Jn))
            dev = max(dev, e)
            assert e <= FWD_BOUND[kind], (cases.gid(g), precision, b, t, e)
    assert 4 * left_out <= total, (cases.gid(g), left_out, total)
    print(f"{cases.gid(g)} precision={precision}: forward deviation {dev:.3e}, {left_out} of {total} trials left out")
    worst[cases.gid(g)] = dev


@pytest.mark.parametrize("key", cases.FULL_MODELS + cases.WIDE_MODELS)
def test_forward_trials_match_oracle_fp64(kctx, key):
    worst = {}
    for g in _forward_groups(key):
        _check_forward(kctx, g, 0, "fp64", worst)
    warnings.warn(f"fp64 forward sweep, {key}: largest deviation {max(worst.values()):.3g}")


@pytest.mark.parametrize("precision,kind", [(1, "fp64"), (2, "fp32")])
@pytest.mark.parametrize("key", cases.F32_MODELS + ["tree4"])
def test_forward_trials_match_oracle_reduced_precision(kctx, key, precision, kind):
    """precision 1 (fp32 Jacobians and Riccati sweep, fp64 rollouts) and 2 (mixed: fp32 rollout dynamics) against
    the fp64 oracle run with the GPU's own K, d"""
    worst = {}
    for g in [g for g in _forward_groups(key) if g.cost != "default" and g.cost != "qfstart"]:
        _check_forward(kctx, g, precision, kind, worst)
    warnings.warn(f"forward sweep at precision {precision}, {key}: largest deviation {max(worst.values()):.3g}")
