"""Closed loop on the device with a plant that is not the controller's model: MPC steps / s with and without per-instance
plant inertials, and the device time of the rollout kernel between two MPC steps.

The problem is the `sine` workload of bench.py (Panda, goal-reaching rows, sine_wave_configuration_space references); every step is
feedback_rollout(n_sub, dt / n_sub) + mpc_step(k, 10, first=2).  Three plants: none (k_feedback_rollout on the model), the
nominal model as a plant, and seeded perturbed plants with a payload on instance 1 (both k_plant_rollout).  The kernel time is
agx_ocp_time_kernel(8): hipEvents around `--launches` back-to-back launches after a warm-up launch, `--repeats` times per
plant, the three plants in turn, so that each plant's figures sample the same stretch of time.  One JSON line per plant.

  python scripts/bench_plant_mismatch.py [--batch 1024] [--horizon 20] [--steps 100] [--warmup 10] [--n-sub 10]
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

PLANTS = ("none", "nominal", "perturbed")


def make(B, T, n_points, plant):
    table = rt.panda_table(0.1)
    tcp = table.frame_id("panda_hand_tcp")
    po = _abi.PackedOcp(7, [0.01] * T, *workloads.goal_reaching_rows(tcp))
    hip = backend.HipOcp(table, po, B)
    q0, amp, puls, scale, t0 = workloads.sine_batch_params(B, lower=table.lower_position_limit, upper=table.upper_position_limit)
    w = workloads.SINE_WEIGHTS
    hip.sine_trajectory(n_points, 0.01, q0, amp, puls, scale, t0, w["w_q"], w["w_qdot"], w["w_effort"], w["w_pose"], tcp)
    if plant == "nominal":
        hip.set_plant_inertials(*workloads.stack_inertials([table] * B))
    elif plant == "perturbed":
        hip.set_plant_inertials(*workloads.stack_inertials(workloads.plant_tables(table, B, seed=1, rel=0.1, payload=(2.0, (0.0, 0.0, 0.1)))))
    return hip


def closed_loop(hip, steps, warmup, n_sub):
    hip.mpc_step(0, 10, first=True)
    for k in range(1, warmup + 1):
        hip.feedback_rollout(n_sub, 0.01 / n_sub)
        hip.mpc_step(k, 10, first=2)
    hip.sync()
    t_start = time.perf_counter()
    for k in range(warmup + 1, warmup + 1 + steps):
        hip.feedback_rollout(n_sub, 0.01 / n_sub)
        hip.mpc_step(k, 10, first=2)
    hip.sync()
    elapsed = time.perf_counter() - t_start
    st = hip.download(want_K=False)[3]
    return steps / elapsed, bool(np.all(np.isfinite(st["cost"])))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--horizon", type=int, default=20)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--n-sub", type=int, default=10)
    ap.add_argument("--launches", type=int, default=20, help="timed launches of the rollout kernel per repeat")
    ap.add_argument("--repeats", type=int, default=5)
    args = ap.parse_args()
    n_points = args.warmup + args.steps + args.horizon + 3
    handles = {p: make(args.batch, args.horizon, n_points, p) for p in PLANTS}
    rate, finite = {}, {}
    for p in PLANTS:
        rate[p], finite[p] = closed_loop(handles[p], args.steps, args.warmup, args.n_sub)
    # the kernel alone, at the state the closed loop left (which = 8 is 10 sub-steps of 1 ms whatever --n-sub says)
    ms = {p: [] for p in PLANTS}
    for _ in range(args.repeats):
        for p in PLANTS:
            ms[p].append(handles[p].time_kernel(8, args.launches))
    for p in PLANTS:
        t = np.array(ms[p])
        print(json.dumps({"plant": p, "kernel": "k_feedback_rollout" if p == "none" else "k_plant_rollout", "batch": args.batch,
                          "horizon": args.horizon, "steps": args.steps, "n_sub": args.n_sub, "steps_per_s": rate[p],
                          "instance_steps_per_s": args.batch * rate[p], "finite": finite[p], "rollout_ms_mean": float(t.mean()),
                          "rollout_ms_min": float(t.min()), "rollout_ms_max": float(t.max()), "rollout_ms_repeats": [float(v) for v in t],
                          "launches_per_repeat": args.launches}), flush=True)
        handles[p].close()


if __name__ == "__main__":
    main()
