"""The reference of the dynamics kernel tests (oracle/rbd.py in long double on tests/dyn_cases.py's models), checked
on the CPU: not the kernel.  oracle/rbd.py restates the recursions the kernels implement, and the reference
project's own outputs pin it on planar arms only (test_oracle_golden.py): on a model with a branch, a spatial
offset or a prismatic joint the oracle and a kernel can be wrong together.  So the reference is held to conditions
that do not come from a restatement:

(a) identities, long double, every model: M assembled from RNEA columns (qd = 0, gravity = 0, qdd = e_i) is
    symmetric, |M Minv - I| <= 1e-12 and |RNEA(q, qd, FD(q, qd, u)) - u| <= 1e-12 (absolute).
    Measured: asymmetry <= 1.8e-18 max|M| (tree7), M Minv - I <= 1.6e-15 and residual <= 2.9e-15 (arm12).
(b) the analytic Jacobians A, B of the Euler step equal the 6th-order central difference of rbd.euler (h = 1e-3,
    coefficients 3/4, -3/20, 1/60), max|diff| <= 1e-10 max(1, max|A|).  Measured: <= 6.9e-13 relative, 1.9e-11
    absolute (spatial12).  With the reference project's revolute-only fxS (delta = -X^T crm(f) S) in
    place, every model with a prismatic joint misses by 0.25 (tree12) .. 4.9 (spatial12) relative, and every
    revolute-only model is unchanged (<= 8.5e-14): only the dq columns of prismatic joints differ.
(c) the long-double run agrees with the reference project's own outputs (dyn_arm2 / arm3 / arm6fix.npz) within
    test_oracle_golden.py's bounds.
(d) mutations of the fp64 oracle, applied through a test-local patch: what the zoo sees and planar arms cannot.
    The error is the largest of rel(qdd), rel(Minv), rel(A) against the long-double reference; "caught" is
    > 1e-6, "at rounding" is <= 1e-10 (fp64's 1.1e-16 times the arms' condition, max|Minv| = 825 on arm12, with
    decades to spare: measured <= 5.1e-13, arm12).
      old-fxS      delta = -X^T crm(f) S.  Caught by every model with a prismatic joint: spatial2, spatial5,
                   spatial7, spatial8, spatial12, tree4, tree7, tree9, tree12 (0.25 .. 1.8).  revolute6 and the
                   planar arms keep their values (signs of zeros apart).
      chain-subtree  minv's subtree list replaced by the chain rule s >= j.  This mutation has NO effect on any
                   model, tree or chain: column s of F[j] is exactly zero for s outside subtree(j) (it is only ever
                   filled from children c with s in subtree(c)), so the extra terms add Dinv * 0 and U * 0.  The
                   subtree list (and the kernels' subtree bit mask, in_subtree) is an operation count saving, not
                   a condition of correctness, and no test on any model can catch its replacement by s >= j; the
                   test asserts that the mutated Minv is the unmutated one, value for value.
      chain-instance  the chain rule for both of the chain instance's shortcuts, parent(j) = j - 1 and s >= j
                   (what dispatching CHAIN = true on a branched model would compute).  Caught by every tree:
                   tree4, tree7, tree9, tree12 (1.6 .. 4.5); chains cannot see it.
      late-root    a joint on the base at j > 0 treated as the child of j - 1.  Caught by the two-root trees
                   tree7, tree9, tree12 (2.6 .. 53); every other model has no such joint.
"""
import dataclasses

import numpy as np
import pytest

import dyn_cases as dc
from conftest import arm_model, golden
from oracle import rbd

HP = dc.HP
# the reference's format: x87 extended precision (64-bit significand)
assert np.finfo(HP).eps < 2e-19, "long double is not an extended-precision format on this host"

K_CPU = 3


def _hp_state(key):
    x, u = dc.states(key, K_CPU)
    return np.asarray(x, dtype=HP), np.asarray(u, dtype=HP)


# ------------------------------------------------------------------------------------------------ (a)
@pytest.mark.parametrize("key", dc.ALL_MODELS)
def test_identities_in_long_double(key):
    m = dc.model(key)
    n = m.n
    x, u = _hp_state(key)
    q, qd = x[:, :n], x[:, n:]
    zero = np.zeros_like(q)
    cols = []
    for i in range(n):
        e = zero.copy()
        e[:, i] = 1
        c = rbd.rnea(m, q, zero, e, gravity=0.0)[0]
        assert c.dtype == HP
        cols.append(c)
    M = np.stack(cols, axis=2)
    Mi = rbd.minv(m, q)
    qdd = rbd.forward_dynamics(m, x, u)
    res = rbd.rnea(m, q, qd, qdd)[0] - u
    assert Mi.dtype == HP and qdd.dtype == HP and res.dtype == HP
    asym = float(np.max(np.abs(M - np.transpose(M, (0, 2, 1)))) / np.max(np.abs(M)))
    eye = float(np.max(np.abs(M @ Mi - np.eye(n, dtype=HP))))
    r = float(np.max(np.abs(res)))
    print(f"{key}: asymmetry {asym:.2e} max|M|, |M Minv - I| {eye:.2e}, |RNEA(FD) - u| {r:.2e}")
    assert asym <= 1e-17, (key, asym)   # a symmetric M computed in another order: a few long-double ulps (1.1e-19)
    assert eye <= 1e-12 and r <= 1e-12, (key, eye, r)


def test_every_output_takes_the_precision_of_its_inputs():
    """long double in, long double out (every routine, every output); float32 in, float32 out; float64 keeps the
    model object itself (no copy, the operations of the fp64 oracle are unchanged)"""
    m = dc.model("tree7")
    n = m.n
    x64, u64 = dc.states("tree7", K_CPU)
    assert rbd.cast_model(m, np.float64) is m
    for dtype in (HP, np.float32, np.float64):
        x, u = x64.astype(dtype), u64.astype(dtype)
        mc = rbd.cast_model(m, dtype)
        for k in ("S", "X0", "Xa", "Xb", "I"):
            assert getattr(mc, k).dtype == np.dtype(dtype)
        q, qd = x[:, :n], x[:, n:]
        qdd = rbd.forward_dynamics(m, x, u)
        outs = list(rbd.rnea(m, q, qd, qdd)) + list(rbd.rnea(m, q, qd, None)) + [
            qdd, rbd.rnea_grad(m, q, qd, qdd), rbd.minv(m, q), rbd.forward_dynamics_gradient(m, x, u),
            rbd.euler(m, x, u, dc.DT), *rbd.euler_gradient(m, x, u, dc.DT)]
        for o in outs:
            assert o.dtype == np.dtype(dtype), (dtype, o.dtype)
    # the three precisions are the same function: float32 and float64 sit at their own rounding from long double
    ref = dc.evaluate(m, x64, u64, HP)
    for dtype, cap in ((np.float64, 1e-11), (np.float32, 1e-2)):
        got = dc.evaluate(m, x64.astype(dtype), u64.astype(dtype), dtype)
        hp_same_inputs = ref if dtype == np.float64 else dc.evaluate(m, x64.astype(dtype), u64.astype(dtype), HP)
        for k in dc.QUANTITIES:
            assert dc.rel(got[k], hp_same_inputs[k]) <= cap, (dtype, k, dc.rel(got[k], hp_same_inputs[k]))


# ------------------------------------------------------------------------------------------------ (b)
FD_H = HP(1) / 1000
FD_COEF = (HP(3) / 4, -HP(3) / 20, HP(1) / 60)


def _central_difference(m, x, u):
    """the 6th-order central difference of rbd.euler in long double: (A_fd, B_fd); every perturbed state in one
    batch"""
    K, nx = x.shape
    nz = nx + m.n
    z = np.concatenate([x, u], axis=1)
    zs = []
    for i in range(nz):
        for k in (1, 2, 3):
            for sgn in (1, -1):
                zp = z.copy()
                zp[:, i] += sgn * k * FD_H
                zs.append(zp)
    zs = np.concatenate(zs, axis=0)
    f = rbd.euler(m, zs[:, :nx], zs[:, nx:], dc.DT).reshape(nz, 3, 2, K, nx)
    J = sum(c * (f[:, k, 0] - f[:, k, 1]) for k, c in enumerate(FD_COEF)) / FD_H   # [nz][K][nx]
    J = np.transpose(J, (1, 2, 0))
    return J[:, :, :nx], J[:, :, nx:]


def _fd_miss(key):
    m = dc.model(key)
    x, u = _hp_state(key)
    A, B = rbd.euler_gradient(m, x, u, dc.DT)
    assert A.dtype == HP and B.dtype == HP
    Af, Bf = _central_difference(m, x, u)
    scale = max(1.0, float(np.max(np.abs(A))))
    return max(float(np.max(np.abs(A - Af))), float(np.max(np.abs(B - Bf)))), scale


@pytest.mark.parametrize("key", dc.ALL_MODELS)
def test_jacobians_equal_the_finite_difference_of_the_step(key):
    miss, scale = _fd_miss(key)
    print(f"{key}: max|[A B] - fd| = {miss:.2e} = {miss / scale:.2e} max(1, max|A|)")
    assert miss <= 1e-10 * scale, (key, miss, scale)


# ------------------------------------------------------------------------------------------------ (c)
def _rel1(a, b):
    """test_oracle_golden.py's measure"""
    return float(np.max(np.abs(np.asarray(a, dtype=HP) - np.asarray(b, dtype=HP)))) / max(1.0, float(np.max(np.abs(b))))


@pytest.mark.parametrize("name", ["arm2", "arm3", "arm6fix"])
def test_long_double_run_matches_the_reference_projects_outputs(name):
    d = golden(f"dyn_{name}.npz")
    m = arm_model(name)
    n = m.n
    x, u, dt = d["x"].astype(HP), d["u"].astype(HP), float(d["dt"])
    q, qd = x[:, :n], x[:, n:]
    assert _rel1(rbd.minv(m, q), d["Minv"]) < 1e-11
    assert _rel1(rbd.rnea(m, q, qd, None)[0], d["c"]) < 1e-11
    assert _rel1(rbd.forward_dynamics(m, x, u), d["qdd"]) < 1e-10
    assert _rel1(rbd.forward_dynamics_gradient(m, x, u), d["dqdd"]) < 1e-9
    assert _rel1(rbd.rnea_grad(m, q, qd, d["qdd"].astype(HP)), d["dc_du"]) < 1e-9
    assert _rel1(rbd.euler(m, x, u, dt), d["xnext"]) < 1e-11
    A, B = rbd.euler_gradient(m, x, u, dt)
    assert A.dtype == HP
    assert _rel1(A, d["A"]) < 1e-10
    assert _rel1(B, d["B"]) < 1e-11


# ------------------------------------------------------------------------------------------------ (d)
CAUGHT, ROUNDING = 1e-6, 1e-10


def _old_fxS(S, f):
    """the reference project's term (RBDReference.py:94-97)"""
    return -rbd.mxS(S, f)


def _chain_subtree(m):
    return dataclasses.replace(m, subtree=[list(range(j, m.n)) for j in range(m.n)])


def _chain_instance(m):
    return dataclasses.replace(_chain_subtree(m), parent=np.arange(-1, m.n - 1, dtype=m.parent.dtype))


def _late_root(m):
    parent = m.parent.copy()
    for j in range(1, m.n):
        if parent[j] == -1:
            parent[j] = j - 1
    return dataclasses.replace(m, parent=parent)


def _miss64(key, m):
    """the fp64 oracle on model m against the long-double reference of the zoo's model"""
    x, u = dc.states(key, K_CPU)
    got, ref = dc.evaluate(m, x, u, np.float64), dc.reference(key, K_CPU)
    return max(dc.rel(got[k], ref[k]) for k in ("qdd", "Minv", "A"))


@pytest.mark.parametrize("key", dc.ALL_MODELS)
def test_mutation_old_fxS(key, monkeypatch):
    dc.reference(key, K_CPU)   # (cached) before the patch: the reference is the unmutated oracle's
    monkeypatch.setattr(rbd, "fxS", _old_fxS)
    e = _miss64(key, dc.model(key))
    print(f"{key}: old fxS misses the reference by {e:.2e}")
    if dc.has_prismatic(key):
        assert e > CAUGHT, (key, e)
    else:
        assert e <= ROUNDING, (key, e)
    miss, scale = _fd_miss(key)   # and (b) fails on it, on exactly these models
    print(f"{key}: old fxS, (b) measures {miss / scale:.2e}")
    assert (miss > 1e-10 * scale) == dc.has_prismatic(key), (key, miss, scale)


@pytest.mark.parametrize("key", dc.ALL_MODELS)
def test_mutation_chain_rule_for_the_subtree_list_changes_nothing(key):
    """see the module docstring: the columns the chain rule adds are exact zeros"""
    m = dc.model(key)
    x, _ = dc.states(key, K_CPU)
    a, b = rbd.minv(_chain_subtree(m), x[:, :m.n]), rbd.minv(m, x[:, :m.n])
    assert np.array_equal(a, b), key
    assert _miss64(key, _chain_subtree(m)) <= ROUNDING


@pytest.mark.parametrize("key", dc.ALL_MODELS)
def test_mutation_chain_instance_on_a_tree(key):
    e = _miss64(key, _chain_instance(dc.model(key)))
    print(f"{key}: the chain instance misses the reference by {e:.2e}")
    if dc.is_tree(key):
        assert e > CAUGHT, (key, e)
    else:
        assert e <= ROUNDING, (key, e)


@pytest.mark.parametrize("key", dc.ALL_MODELS)
def test_mutation_late_root_as_a_child(key):
    e = _miss64(key, _late_root(dc.model(key)))
    print(f"{key}: a late root as the child of j - 1 misses the reference by {e:.2e}")
    if dc.has_late_root(key):
        assert e > CAUGHT, (key, e)
    else:
        assert e <= ROUNDING, (key, e)


def test_the_zoo_is_what_it_says():
    assert [k for k in dc.ALL_MODELS if dc.has_late_root(k)] == ["tree7", "tree9", "tree12"]
    assert [k for k in dc.ALL_MODELS if dc.is_tree(k)] == ["tree7", "tree9", "tree12", "tree4"]
    assert [k for k in dc.ALL_MODELS if dc.has_prismatic(k)] == [
        "spatial2", "spatial5", "spatial7", "spatial8", "spatial12", "tree7", "tree9", "tree12", "tree4"]
    assert list(dc.model("tree9").parent) == [-1, 0, 1, 0, 3, 4, -1, 6, 6]
    assert list(np.flatnonzero(dc.model("tree9").jtype)) == [4, 8]
    assert list(dc.model("tree12").parent) == [-1, 0, 1, 2, 0, 4, 5, 5, -1, 8, 9, 8]
    assert list(np.flatnonzero(dc.model("tree12").jtype)) == [6, 11]
    for key in dc.GENERATED:
        m = dc.model(key)
        for j in range(m.n):   # spatial: the out-of-plane blocks of I and of X(0) are populated
            assert np.count_nonzero(m.I[j]) == 24, (key, j)   # full but for the skew blocks' and m 1's zeros
            assert np.count_nonzero(m.X0[j] + m.Xa[j]) >= 27, (key, j)
