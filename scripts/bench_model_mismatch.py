"""Closed loop on the device with ONE plant and several controller models: the Panda with a payload on link 7 is the plant of
every instance (set_plant_inertials); the controller solves with the nominal table (a handle that never had per-instance
inertials), with the payload in its model, or with seeded +-10 % perturbed models, one per instance (set_model_inertials).

The loop is that of scripts/bench_plant_mismatch.py (the `sine` workload of bench.py; every step is
feedback_rollout(n_sub, dt / n_sub) + mpc_step(k, 10, first=2)).  Per group: MPC steps / s over `--steps` steps without any
download, then the tracking error over `--err-steps` further steps: the mean over steps and instances of |q_plant - q_ref| (rad,
joint space, Euclidean norm) at the sample the step starts from.  One JSON line per group.

  python scripts/bench_model_mismatch.py [--batch 1024] [--horizon 20] [--steps 100] [--warmup 10] [--err-steps 50] [--n-sub 10]
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

GROUPS = ("nominal", "payload", "perturbed")
PAYLOAD = (2.0, (0.0, 0.0, 0.1))


def make(B, T, n_points, group):
    table = rt.panda_table(0.1)
    tcp = table.frame_id("panda_hand_tcp")
    po = _abi.PackedOcp(7, [0.01] * T, *workloads.goal_reaching_rows(tcp))
    hip = backend.HipOcp(table, po, B)
    q0, amp, puls, scale, t0 = workloads.sine_batch_params(B, lower=table.lower_position_limit, upper=table.upper_position_limit)
    w = workloads.SINE_WEIGHTS
    hip.sine_trajectory(n_points, 0.01, q0, amp, puls, scale, t0, w["w_q"], w["w_qdot"], w["w_effort"], w["w_pose"], tcp)
    loaded = workloads.plant_tables(table, 2, seed=1, payload=PAYLOAD)[1]
    hip.set_plant_inertials(*workloads.stack_inertials([loaded] * B))
    if group == "payload":
        hip.set_model_inertials(*workloads.stack_inertials([loaded] * B))
    elif group == "perturbed":  # entry 0 of plant_tables is the nominal table: B + 1 tables, the first dropped
        hip.set_model_inertials(*workloads.stack_inertials(workloads.plant_tables(table, B + 1, seed=1, rel=0.1)[1:]))
    return hip


def closed_loop(hip, steps, warmup, err_steps, n_sub):
    hip.mpc_step(0, 10, first=True)
    k = 1
    for _ in range(warmup):
        hip.feedback_rollout(n_sub, 0.01 / n_sub)
        hip.mpc_step(k, 10, first=2)
        k += 1
    hip.sync()
    t_start = time.perf_counter()
    for _ in range(steps):
        hip.feedback_rollout(n_sub, 0.01 / n_sub)
        hip.mpc_step(k, 10, first=2)
        k += 1
    hip.sync()
    rate = steps / (time.perf_counter() - t_start)
    err = []
    nv = hip.nv
    for _ in range(err_steps):
        hip.feedback_rollout(n_sub, 0.01 / n_sub)
        err.append(np.linalg.norm(hip.download_x0()[:, :nv] - hip.traj_point(k)[0], axis=1))
        hip.mpc_step(k, 10, first=2)
        k += 1
    st = hip.download(want_K=False)[3]
    return rate, np.array(err), bool(np.all(np.isfinite(st["cost"])))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--horizon", type=int, default=20)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--err-steps", type=int, default=50)
    ap.add_argument("--n-sub", type=int, default=10)
    args = ap.parse_args()
    n_points = args.warmup + args.steps + args.err_steps + args.horizon + 3
    for group in GROUPS:
        hip = make(args.batch, args.horizon, n_points, group)
        rate, err, finite = closed_loop(hip, args.steps, args.warmup, args.err_steps, args.n_sub)
        hip.close()
        print(json.dumps({"controller_model": group, "plant": "panda + 2 kg at (0, 0, 0.1) of link 7", "batch": args.batch, "horizon": args.horizon,
                          "steps": args.steps, "n_sub": args.n_sub, "steps_per_s": rate, "instance_steps_per_s": args.batch * rate,
                          "tracking_error_mean_rad": float(err.mean()), "tracking_error_max_rad": float(err.max()),
                          "tracking_error_last_step_mean_rad": float(err[-1].mean()), "err_steps": args.err_steps, "finite": finite}), flush=True)


if __name__ == "__main__":
    main()
