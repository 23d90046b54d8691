"""MPC steps / s on the device with the general cost rows (ResidualModelControlGrav, ResidualModelFrameVelocity) on large models,
and what k_general_rows_wg / k_node_kkt_big_gen cost next to k_calc_qp_wg / k_node_kkt_big.

Two models: the 30-joint humanoid (B = 512, T = 50) and the Panda with unlocked fingers (9 joints at the 16-joint capacity,
B = 256, T = 50).  For each the rows {State, Control, FramePlacement} alone, then plus ControlGrav, plus FrameVelocity, plus both,
on a resident sine trajectory.  One JSON line per leg: batch and instance steps / s, and the per-launch times of the derivative
pass (kernel 0 of agx_ocp_time_kernel: k_calc_qp_wg, with general rows followed by k_general_rows_wg) and of the step head
(kernel 2: k_node_kkt_big or k_node_kkt_big_gen, then k_sqp_head); the difference to the first leg is what the new kernels add.

The resident generators leave the activation weights of the two rows at zero (they have no reference for them), so in these
legs the rows are INERT: they are evaluated -- the kernels run the instruction stream they run with any weights -- but do not
move the solution; the SQP iteration counts of the four legs are equal and the steps / s differ by the kernels' time alone.
The legs "host_base" / "host_both" are the representative ones: a host reference tile with seeded random references and
NON-ZERO weights on every row (workloads.random_goal_problem), the same cold solve (10 iterations at most) repeated from the
same warm start; they report solves / s and the SQP iterations the rows cost.

Per-kernel times: run one leg under a kernel trace in a run of its own,
  rocprofv3 --kernel-trace --stats -d <dir> -- python scripts/bench_general_rows.py --models humanoid30 --legs both --repeat 1
and read k_calc_qp_wg, k_general_rows_wg, k_node_kkt_big / k_node_kkt_big_gen out of the kernel statistics.

  python scripts/bench_general_rows.py [--steps 30] [--warmup 5] [--repeat 3] [--models humanoid30 panda_fingers]

--base-only runs the first leg alone (for comparing two builds of the library, AGX_LIB, on the leg without general rows).
"""
from __future__ import annotations

import argparse
import json
import pathlib
import sys
import time

import numpy as np

ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

from agimus_controller_amd import _abi, backend, workloads  # noqa: E402
from agimus_controller_amd.factory import robot_tables as rt  # noqa: E402


MODELS = {"humanoid30": (rt.humanoid30_table, 512), "panda_fingers": (rt.panda_fingers_table, 256)}
LEGS = [("base", False, False), ("control_grav", True, False), ("frame_velocity", False, True), ("both", True, True)]


def rows_of(frame, grav, fvel):
    running, terminal = workloads.goal_reaching_rows(frame)
    running, terminal = list(running), list(terminal)
    if fvel:
        running.append(_abi.RowSpec(_abi.RES_FRAME_VELOCITY, frame=frame, frame_b=2, name="ee_velocity"))
        terminal.append(_abi.RowSpec(_abi.RES_FRAME_VELOCITY, frame=frame, frame_b=2, name="ee_velocity"))
    if grav:
        running.append(_abi.RowSpec(_abi.RES_CONTROL_GRAV, name="ctrl_grav"))
    return running, terminal


def run(model, leg, grav, fvel, T, steps, warmup):
    make, B = MODELS[model]
    table = make()
    nv = table.nv
    frame = table.frame_id("panda_hand_tcp") if "panda_hand_tcp" in table.frame_names else len(table.frame_names) - 1
    running, terminal = rows_of(frame, grav, fvel)
    po = _abi.PackedOcp(nv, [0.01] * T, running, terminal, termination_tolerance=1e-3)
    hip = backend.HipOcp(table, po, B)
    general = bool(getattr(hip, "general_rows", False))  # (a library without the entry point: the base leg of an older build)
    q0, amp, puls, scale, t0 = workloads.sine_batch_params(B, nv=nv, q0=np.zeros(nv))
    hip.sine_trajectory(warmup + steps + T + 2, 0.01, q0, amp, puls, scale, t0, np.full(nv, 1.0), np.full(nv, 0.1), np.full(nv, 1e-3),
                        np.full(6, 2.0), frame)
    iters = []
    for k in range(warmup):
        hip.mpc_step(k, 10, first=(k == 0))
        hip.download_first(copy=False)
    hip.sync()
    t_start = time.perf_counter()
    for k in range(warmup, warmup + steps):
        hip.mpc_step(k, 10, first=False)
        iters.append(float(hip.download_first(copy=False)[3]["iter"].mean()))
    hip.sync()
    elapsed = time.perf_counter() - t_start
    out = {"model": model, "nv": nv, "leg": leg, "general_rows": general, "batch": B, "horizon": T, "steps": steps, "steps_per_s": steps / elapsed,
           "instance_steps_per_s": B * steps / elapsed, "ms_per_step": 1e3 * elapsed / steps, "mean_sqp_iter": float(np.mean(iters)),
           "derivative_pass_ms": hip.time_kernel(0, 20), "step_head_ms": hip.time_kernel(2, 20)}
    hip.close()
    return out


def run_host(model, leg, grav, fvel, T, reps):
    """Cold solves on a host tile whose general rows carry weights."""
    make, B = MODELS[model]
    table = make()
    nv = table.nv
    frame = table.frame_id("panda_hand_tcp") if "panda_hand_tcp" in table.frame_names else len(table.frame_names) - 1
    po0, ref, x0, xs, us = workloads.random_goal_problem(table, T, 0.01, B, seed=3, frame=frame, rows=rows_of(frame, grav, fvel))
    po = _abi.PackedOcp(nv, [0.01] * T, po0.running, po0.terminal, termination_tolerance=1e-3)
    hip = backend.HipOcp(table, po, B)
    hip.set_refs(ref)
    elapsed, iters = 0.0, None
    for r in range(reps + 1):  # the first one warms up
        hip.upload_x0(x0)
        hip.upload_warmstart(xs, us)
        hip.sync()
        t_start = time.perf_counter()
        hip.solve_resident(10)
        hip.sync()
        if r:
            elapsed += time.perf_counter() - t_start
        iters = hip.download(want_K=False)[3]["iter"]
    out = {"model": model, "nv": nv, "leg": leg, "general_rows": bool(getattr(hip, "general_rows", False)), "batch": B, "horizon": T, "solves": reps,
           "solves_per_s": reps / elapsed, "instance_solves_per_s": B * reps / elapsed, "ms_per_solve": 1e3 * elapsed / reps,
           "mean_sqp_iter": float(np.mean(iters)), "max_sqp_iter": int(np.max(iters))}
    hip.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--models", nargs="+", default=list(MODELS), choices=list(MODELS))
    ap.add_argument("--horizon", type=int, default=50)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--base-only", action="store_true")
    ap.add_argument("--legs", nargs="+", default=None, help="a subset of: base control_grav frame_velocity both host_base host_both")
    args = ap.parse_args()
    names = ["base"] if args.base_only else (args.legs or [n for n, _, _ in LEGS] + ["host_base", "host_both"])
    for model in args.models:
        for leg, grav, fvel in LEGS:
            if leg not in names:
                continue
            for rep in range(args.repeat):
                out = run(model, leg, grav, fvel, args.horizon, args.steps, args.warmup)
                out["repeat"] = rep
                print(json.dumps(out), flush=True)
        for leg, both in (("host_base", False), ("host_both", True)):
            if leg in names:
                for rep in range(args.repeat):
                    out = run_host(model, leg, both, both, args.horizon, 10)
                    out["repeat"] = rep
                    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
