"""The solver state machine's scalar rules as the device kernels call them (csrc/tmpc_state.h: the step
outcome, the two line-search trial tests, the outer loop's exit rule) in a stand-alone program
(host_state_check.cpp, its own main) built with the host compiler's address and undefined-behaviour
sanitizers and without floating-point contraction, compared exactly -- bit for bit -- with the oracle's
statement of the same rules (oracle/state.py, which oracle.sqp.sqp and oracle.ilqr.ilqr run on) and replayed
over the reference's recorded SQP traces.  No GPU, nothing loaded into Python."""
import glob
import itertools
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN, ROOT
from oracle import state
from oracle.sqp import default_options


@pytest.fixture(scope="module")
def check(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("clang++") or shutil.which("c++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = tmp_path_factory.mktemp("host_state") / "host_state_check"
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-ffp-contract=off",
                        "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        "-I", os.path.join(ROOT, "trajoptmpcreference_amd", "csrc"),
                        os.path.join(ROOT, "tests", "host_state_check.cpp"), "-o", str(exe)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]

    def run(lines):
        """The program's answers to `lines` (each a kind and its numbers): one list of fields per line."""
        text = "".join(" ".join([ln[0]] + [float(v).hex() if isinstance(v, float) else str(int(v)) for v in ln[1:]])
                       + "\n" for ln in lines)
        r = subprocess.run([str(exe)], input=text, capture_output=True, text=True)
        assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
        out = [ln.split() for ln in r.stdout.splitlines()]
        assert [o[0] for o in out] == [ln[0] for ln in lines]
        return [o[1:] for o in out]
    return run


def opts_line(o):
    return ("opts", float(o["exit_tolerance_SQP_DDP"]), float(o["alpha_factor_SQP_DDP"]), float(o["alpha_min_SQP_DDP"]),
            float(o["rho_factor_SQP_DDP"]), float(o["rho_min_SQP_DDP"]), float(o["rho_max_SQP_DDP"]),
            float(o["rho_init_SQP_DDP"]), float(o["expected_reduction_min_SQP_DDP"]),
            float(o["expected_reduction_max_SQP_DDP"]), 10.0, int(o["max_iter_SQP_DDP"]))


def same(got_hex, want):
    """Bit equality of a printed hex float with the oracle's number (any NaN equals any NaN)."""
    got, want = float.fromhex(got_hex), float(want)
    return (math.isnan(got) and math.isnan(want)) or got.hex() == want.hex()


def check_steps(check, o, cases):
    """cases: (error, deltaJ, it, rho, drho) under options o, each against oracle.state.step_outcome."""
    got = check([opts_line(o)] + [("step", int(e), float(dj), int(it), float(rho), float(drho))
                                  for e, dj, it, rho, drho in cases])[1:]
    for (e, dj, it, rho, drho), g in zip(cases, got):
        trace_rho, rho_n, drho_n, code, it_n = state.step_outcome(o, e, dj, it, rho, drho)
        assert same(g[0], trace_rho) and same(g[1], rho_n) and same(g[2], drho_n), (e, dj, it, rho, drho, g)
        done = code != 0
        assert [int(v) for v in g[3:]] == [code, int(done), it_n, int(not e and not done)], (e, dj, it, rho, drho, g)


def test_step_outcome_grid(check):
    o0 = default_options()
    tol, huge = o0["exit_tolerance_SQP_DDP"], dict(o0, max_iter_SQP_DDP=1000)
    # every (rho, drho) reached from (rho_init, 1) by up to 8 errors / accepts in any order
    states = {(float(o0["rho_init_SQP_DDP"]), 1.0)}
    for n in range(1, 9):
        for seq in itertools.product((False, True), repeat=n):
            rho, drho = o0["rho_init_SQP_DDP"], 1
            for e in seq:
                _, rho, drho, _, _ = state.step_outcome(huge, e, 1.0, 0, rho, drho)
            states.add((float(rho), float(drho)))
    assert any(r > o0["rho_max_SQP_DDP"] for r, _ in states)                       # past rho_max
    assert any(r == o0["rho_min_SQP_DDP"] and d < 1e-3 for r, d in states)         # clamped at rho_min
    exits = set()
    for max_iter in (1, 2, 20):
        o = dict(o0, max_iter_SQP_DDP=max_iter)
        its = sorted({it for it in (0, max_iter - 2, max_iter - 1) if it >= 0})
        cases = [(e, dj, it, rho, drho) for e in (False, True) for dj in (-1.0, 0.0, tol / 2, tol, 1.0) for it in its
                 for rho, drho in sorted(states)]
        check_steps(check, o, cases)
        exits |= {state.step_outcome(o, *c)[3] for c in cases}
    assert exits == {0, 1, 2, 3}


def test_trial_tests(check):
    o = default_options()
    lo, hi, mu = o["expected_reduction_min_SQP_DDP"], o["expected_reduction_max_SQP_DDP"], 10.0
    nan, inf = float("nan"), float("inf")
    # (merit, Jn, cn, D, al) -> accepted; with cn = 0, al = 1 the expected reduction is D and the ratio merit - Jn
    sqp = [((lo, 0.0, 0.0, 1.0, 1.0), True), ((float(hi), 0.0, 0.0, 1.0, 1.0), True),
           ((math.nextafter(lo, 0.0), 0.0, 0.0, 1.0, 1.0), False), ((math.nextafter(hi, inf), 0.0, 0.0, 1.0, 1.0), False),
           ((1.0, 0.0, 0.0, 1.0, 1.0), True),
           ((-1.0, 0.0, 0.0, -1.0, 1.0), False),    # the merit grows; the ratio 1 is in range
           ((1.0, 0.0, 0.0, 0.0, 1.0), False),      # no expected reduction: inf
           ((0.0, 0.0, 0.0, 0.0, 1.0), False),      # ... and 0 / 0
           ((1.0, nan, 0.0, 1.0, 1.0), False),
           ((12.5, 1.0, 0.25, 23.5, 0.5), True),    # merit_new 3.5, expected 0.5 (23.5 - 2.5): ratio 9 / 10.5
           ((12.5, 1.0, 0.25, 3.0, 0.5), False)]    # ... expected 0.5 (3 - 2.5): ratio 36
    # (J, Jn, dV1, dV2, al) -> accepted; with dV1 = -1, dV2 = 0, al = 1 the ratio is J - Jn
    ilqr = [((lo, 0.0, -1.0, 0.0, 1.0), True), ((float(hi), 0.0, -1.0, 0.0, 1.0), True),
            ((math.nextafter(lo, 0.0), 0.0, -1.0, 0.0, 1.0), False),
            ((math.nextafter(hi, inf), 0.0, -1.0, 0.0, 1.0), False),
            ((0.0, 1.0, 1.0, 0.0, 1.0), True),      # a cost increase over a negative denominator: accepted, as it is
            ((1.0, 0.0, 0.0, 0.0, 1.0), False), ((0.0, 0.0, 0.0, 0.0, 1.0), False), ((1.0, nan, -1.0, 0.0, 1.0), False),
            ((5.0, 4.0, -3.0, 1.0, 0.5), True)]     # ratio 1 / (0.5 (3 - 0.5)) = 0.8
    got = check([opts_line(o)] + [("sqp",) + c for c, _ in sqp] + [("ilqr",) + c for c, _ in ilqr])[1:]
    for (c, want), g in zip(sqp, got):
        mn, ratio, acc = state.sqp_trial(o, c[0], c[1], c[2], c[3], c[4], mu)
        assert acc == want and int(g[2]) == int(want), (c, g)
        assert same(g[0], mn) and same(g[1], ratio), (c, g, mn, ratio)
    for (c, want), g in zip(ilqr, got[len(sqp):]):
        dj, ratio, acc = state.ilqr_trial(o, *c)
        assert acc == want and int(g[2]) == int(want), (c, g)
        assert same(g[0], dj) and same(g[1], ratio), (c, g, dj, ratio)


def test_outer_exit_rule(check):
    tol = default_options()["exit_tolerance_softConstraints"]
    cases = [(mc, it, mi, ch) for mc in (tol / 2, tol, 2 * tol, 0.0) for mi, it in ((10, 0), (10, 8), (10, 9), (1, 0))
             for ch in (0, 1)]
    got = check([("outer", float(mc), float(tol), it, mi, ch) for mc, it, mi, ch in cases])
    for (mc, it, mi, ch), g in zip(cases, got):
        ex, it_n = state.outer_exit({"exit_tolerance_softConstraints": tol, "max_iter_softConstraints": mi}, mc, it)
        assert ex == (2 if it == mi - 1 else 1 if mc < tol else 0)
        # (an update that changes no constant ends a pass that would go on: exit 3, oracle.sqp.sqp)
        assert [int(v) for v in g] == [ex, it_n, 3 if ex == 0 and not ch else ex], (mc, it, mi, ch, g)


def test_fixture_replay(check):
    """Every recorded reference SQP trace: the step outcome, fed the trace's line-search flags and cost
    differences, reproduces its rho column row by row, the exit code and the iteration count."""
    o = default_options()
    lines, want = [opts_line(o)], []
    files = [f for f in sorted(glob.glob(os.path.join(GOLDEN, "sqp_*.npz"))) if "tr_rho" in np.load(f).files]
    for f in files:
        d = np.load(f)
        J, ok, tr_rho = d["tr_J"], d["tr_succeeded_line_search"], d["tr_rho"]
        assert len(tr_rho) >= 2 and tr_rho[0] == o["rho_init_SQP_DDP"]
        rho, drho = o["rho_init_SQP_DDP"], 1
        for i in range(1, len(tr_rho)):
            case = (not ok[i], float(J[i - 1] - J[i]), i - 1, float(rho), float(drho))
            lines.append(("step", int(case[0])) + case[1:])
            _, rho, drho, _, _ = state.step_outcome(o, *case)
            last = i == len(tr_rho) - 1
            want.append((os.path.basename(f), i, float(tr_rho[i]), rho, drho, int(d["exit_sqp"]) if last else 0,
                         int(d["sqp_iter"]) if last else i))
    assert len(files) >= 17
    for (name, i, tr_rho, rho, drho, code, it_n), g in zip(want, check(lines)[1:]):
        assert same(g[0], tr_rho) and same(g[1], rho) and same(g[2], drho), (name, i, g, tr_rho, rho, drho)
        assert [int(g[3]), int(g[5])] == [code, it_n], (name, i, g, code, it_n)
