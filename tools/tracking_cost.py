#!/usr/bin/env python3
"""What per-problem, per-knot references (tmpc_set_reference) cost against the fixed goal.

Two shapes, each with the fixed goal, with a reference whose every entry is that goal (R = B, M = N: the same
problems and iterations bit for bit, solved by the tracking kernel instances -- the like-for-like ratio) and with
one per-knot reference per problem (other problems: compare per problem-iteration and per launch only):
  sqp   the headline shape: arm6 N = 64, B = 4096, SQP PCG-SS;
  ilqr  config 3's shape:   arm6 N = 64, B = 4096, iLQR with augmented-Lagrangian torque limits (|u| <= 0.5).
For each it prints one JSON line with the lock-step rate (one batched solve per step), the streamed rate (the
steps' problems through B slots, device-resident) and the per-launch times of k_qp, k_ls_terms,
k_ilqr_backward and k_ilqr_forward from tmpc_kernel_stats (a profiled pass of its own), and last the
tracking / fixed ratios.  The workload is bench.py's (q0 ~ U(-1, 1)^n, qd0 = 0, rollout of u = 0); the
references are tests/tracking_cases.py's (a line between two configurations plus 0.2 sin, M = N).

  python tools/tracking_cost.py [--batch 4096] [--N 64] [--steps 3] [--warmup 1] [--only sqp|ilqr]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

KERNELS = ("qp", "ls_terms", "ilqr_backward", "ilqr_forward")


def reference(n, M, seed, dt):
    rng = np.random.default_rng(100 + seed)
    qa, qb = rng.uniform(-1, 1, n), rng.uniform(-1, 1, n)
    s = np.linspace(0.0, 1.0, M)
    q = qa[:, None] + (qb - qa)[:, None] * s[None, :] + 0.2 * np.sin(2 * np.pi * s)[None, :]
    return np.vstack([q, np.gradient(q, dt, axis=1)])


def problems(model, B, N, dt):
    from oracle import rbd
    n = model.n
    x = np.zeros((B, 2 * n, N))
    for b in range(B):
        x[b, :n, 0] = np.random.default_rng(b).uniform(-1.0, 1.0, n)
    u = np.zeros((B, n, N - 1))
    for k in range(N - 1):
        x[:, :, k + 1] = rbd.euler(model, x[:, :, k], u[:, :, k], dt)
    return x, u


def timed(ctx, fn, steps, warmup):
    for _ in range(warmup):
        fn()
    ctx.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    ctx.synchronize()
    return (time.perf_counter() - t0) / steps


def run(ctx, solver, B, N, dt, x, u, steps, warmup, soft):
    """lock-step and streamed seconds per B problems, and per-launch kernel times"""
    dx, du = ctx.alloc(x.nbytes), ctx.alloc(u.nbytes)
    dxi, dui = ctx.alloc(x.nbytes), ctx.alloc(u.nbytes)
    out = {}
    try:
        ctx.h2d(dxi, x)
        ctx.h2d(dui, u)

        def lockstep():
            if soft:   # the soft-limit state persists across solves of one (B, N): every step from the initial constants
                ctx.set_soft_state(B, N)
            ctx.d2d(dx, dxi, x.nbytes)
            ctx.d2d(du, dui, u.nbytes)
            if solver == "iLQR":
                ctx.ilqr_solve_batch_device(B, N, dt, dx, du)
            else:
                ctx.sqp_solve_batch_device(B, N, dt, dx, du, solver)

        out["lockstep_s"] = timed(ctx, lockstep, steps, warmup)
        # problem-iterations of one batched solve: the tracking problems are other problems, so the rates
        # compare per problem-iteration, the kernels per launch
        out["problem_iterations"] = int(ctx.solve_counters()[0])

        def stream():
            ctx.solve_stream_device(solver, B * steps, B, N, dt, dxi, dui, B)

        stream()
        ctx.synchronize()
        t0 = time.perf_counter()
        stream()
        ctx.synchronize()
        out["stream_s"] = (time.perf_counter() - t0) / steps
        ctx.set_options(profile=1)
        ctx.reset_stats()
        lockstep()
        ctx.synchronize()
        ctx.set_options(profile=0)
        for k in KERNELS:
            cnt, ms = ctx.kernel_stats(k)
            if cnt:
                out[f"{k}_ms_per_launch"] = ms / cnt
                out[f"{k}_launches"] = cnt
    finally:
        for p in (dx, du, dxi, dui):
            ctx.free(p)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--N", type=int, default=64)
    ap.add_argument("--links", type=int, default=6)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--only", choices=["sqp", "ilqr"], default=None)
    a = ap.parse_args()
    from trajoptmpcreference_amd import _native
    from trajoptmpcreference_amd.urdf import parse_urdf, planar_arm_urdf
    n, B, N, dt = a.links, a.batch, a.N, 0.1
    model = parse_urdf(planar_arm_urdf(n))
    x, u = problems(model, B, N, dt)
    refs = np.ascontiguousarray(np.array([reference(n, N, b, dt) for b in range(B)]))
    ctx = _native.Context(0)
    ctx.set_model(model)
    ctx.set_cost_quadratic(np.eye(2 * n), 100.0 * np.eye(2 * n), 0.1 * np.eye(n), np.zeros(2 * n))
    shapes = [("sqp", "PCG-SS", None),
              ("ilqr", "iLQR", {"torque": dict(mode="AUGMENTED_LAGRANGIAN", lb=[-0.5] * n, ub=[0.5] * n)})]
    for name, solver, limits in shapes:
        if a.only and a.only != name:
            continue
        ctx.set_box_limits(limits)
        res = {}
        for goal in ("fixed", "tracking-same-goal", "tracking"):
            ctx.set_reference(refs if goal == "tracking" else np.zeros_like(refs) if goal == "tracking-same-goal" else None)
            r = run(ctx, solver, B, N, dt, x, u, a.steps, a.warmup, limits is not None)
            r.update(shape=name, goal=goal, batch=B, N=N, links=n,
                     lockstep_solves_per_s=B / r["lockstep_s"], stream_solves_per_s=B / r["stream_s"],
                     lockstep_us_per_problem_iteration=1e6 * r["lockstep_s"] / max(1, r["problem_iterations"]))
            res[goal] = r
            print(json.dumps(r), flush=True)
        ctx.set_reference(None)
        for goal in ("tracking-same-goal", "tracking"):
            ratio = {k: res[goal][k] / res["fixed"][k] for k in res["fixed"]
                     if k.endswith(("_s", "_ms_per_launch", "_per_problem_iteration")) and k in res[goal]
                     and res["fixed"][k] > 0}
            print(json.dumps({"shape": name, f"{goal}_over_fixed": ratio}), flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
