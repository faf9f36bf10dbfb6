#!/usr/bin/env python3
"""Latency of the closed-loop MPC step against the on-device loop.

Workload: arm6, N = 64, QP-PCG-SS, fp64, pcg_warm_start, max_iter_SQP_DDP = 4, B problems resident in HBM,
`--steps` MPC steps from the same start every repeat.  Two ways through the same horizon solves and the same
k_mpc_advance launch between them:
  step   `--steps` calls of tmpc_mpc_step_device, each measuring x_meas = the previous call's x_pred (so the
         results are the loop's): the x_meas copy and one host synchronisation per call;
  batch  one tmpc_mpc_batch_device(steps), the loop on the device, one synchronisation at its end.
Per B: a warm-up of each, then `--repeats` timed repeats, the two modes alternating; a host clock around the whole
loop, which ends in a device synchronisation.  Reported per mode: per-step median, min, max and spread
(max - min) in ms.  A last pass with the library's launch timing on (options.profile) reports per mode the
average time of the launch between two solves, "mode:name": the library times it as mpc_shift.

--package-root DIR runs the package and library of another checkout (built there) -- the parent commit's, whose
loop is the yardstick; a checkout without the step entry point runs --modes batch, and one from before the two
modes shared their kernel times its step under the name mpc_advance.  Reads nothing else outside the repository;
prints one JSON line per batch size and, with --out, writes them to a file."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np


def parse(argv=None):
    p = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    p.add_argument("--batches", default="1,64,4096")
    p.add_argument("--steps", type=int, default=20)
    p.add_argument("--repeats", type=int, default=5)
    p.add_argument("--modes", default="step,batch")
    p.add_argument("--links", type=int, default=6)
    p.add_argument("--N", type=int, default=64)
    p.add_argument("--package-root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    p.add_argument("--label", default="this tree")
    p.add_argument("--out", default=None)
    return p.parse_args(argv)


def main(argv=None):
    a = parse(argv)
    sys.path.insert(0, os.path.abspath(a.package_root))
    from trajoptmpcreference_amd import _native
    from trajoptmpcreference_amd.urdf import parse_urdf, planar_arm_urdf
    modes = [m for m in a.modes.split(",") if m]
    n, N, dt, steps, method = a.links, a.N, 0.1, a.steps, "PCG-SS"
    nx, nu = 2 * n, n
    ctx = _native.Context(0)
    ctx.set_model(parse_urdf(planar_arm_urdf(n)))
    ctx.set_cost_quadratic(np.eye(nx), 100 * np.eye(nx), 0.1 * np.eye(nu), np.zeros(nx))
    ctx.set_box_limits(None)
    lines = []
    for B in [int(b) for b in a.batches.split(",")]:
        x0 = np.zeros((B, nx, N))
        for i in range(B):
            x0[i, :n, 0] = np.random.default_rng(1000 + i).uniform(-1.0, 1.0, n)
        u0 = np.zeros((B, nu, N - 1))
        d = {k: ctx.alloc(v) for k, v in dict(x0=x0.nbytes, u0=u0.nbytes, x=x0.nbytes, u=u0.nbytes,
                                              xe=B * nx * (steps + 1) * 8, ue=B * nu * steps * 8, codes=B * steps * 4,
                                              iters=B * steps * 4, su0=B * nu * 8, sxp=B * nx * 8, sst=B * 8).items()}
        ctx.set_options(precision=0, pcg_warm_start=0, profile=0, max_iter_SQP_DDP=4)
        ctx.h2d(d["x0"], x0)
        ctx.h2d(d["u0"], u0)
        ctx.rollout_device(B, N, dt, d["x0"], d["u0"])
        ctx.set_options(pcg_warm_start=1)

        def run(mode):
            ctx.d2d(d["x"], d["x0"], x0.nbytes)
            ctx.d2d(d["u"], d["u0"], u0.nbytes)
            ctx.synchronize()
            t0 = time.perf_counter()
            if mode == "batch":
                ctx.mpc_batch_device(B, N, dt, method, steps, d["x"], d["u"], d["xe"], d["ue"], d["codes"], d["iters"])
            else:
                for s in range(steps):
                    ctx.mpc_step_device(B, N, dt, method, s, d["x"], d["u"], d["sxp"] if s else None, d["su0"],
                                        d["sxp"], d["sst"])
            ctx.synchronize()
            return (time.perf_counter() - t0) * 1e3 / steps

        final = {}
        for m in modes:   # warm-up: code objects loaded, buffers allocated
            run(m)
            xf = np.empty_like(x0)
            ctx.d2h(xf, d["x"])
            final[m] = xf
        times = {m: [] for m in modes}
        for _ in range(a.repeats):
            for m in modes:
                times[m].append(run(m))
        line = dict(tool="mpc_step_latency", label=a.label, links=n, N=N, B=B, steps=steps, repeats=a.repeats,
                    method="QP-" + method, pcg_warm_start=True, precision="fp64", max_iter_SQP_DDP=4, per_step_ms={})
        for m in modes:
            t = times[m]
            line["per_step_ms"][m] = dict(median=statistics.median(t), min=min(t), max=max(t), spread=max(t) - min(t),
                                          runs=t)
        if len(final) == 2:
            line["final_horizon_identical"] = bool(np.array_equal(final["step"], final["batch"]))
        ctx.set_options(profile=1)
        kernels = {}
        for m in modes:
            ctx.reset_stats()
            run(m)
            for name in ("mpc_shift", "mpc_advance"):
                cnt, ms = ctx.kernel_stats(name)
                if cnt:
                    kernels[f"{m}:{name}"] = dict(launches=cnt, avg_ms=ms / cnt)
        line["kernels"] = kernels
        ctx.set_options(profile=0)
        for p in d.values():
            ctx.free(p)
        print(json.dumps(line), flush=True)
        lines.append(line)
    ctx.close()
    if a.out:
        with open(a.out, "w") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
