"""MPC steps / s on the device with many collision-pair COSTS per node (wide cost sets), and k_cost_pairs next to K1.

The problem is the Panda of `bench.py` (sine_wave_configuration_space references, goal-reaching costs: state, control, end-effector
placement) with N soft collision pairs (QuadExp, alpha 0.05, weight 0.1) behind them: the link-7 capsule / sphere pair of the
collision workload, four self-collision pairs, then the five link capsules against further obstacles (capsules, spheres, boxes in
turn).  One JSON line per N: batch and instance steps / s, the per-launch time of the derivative pass (K1 + k_cost_pairs, kernel 0
of agx_ocp_time_kernel) and of k_cost_pairs alone (kernel 9), and the in-situ average of the first trial pass (agx_ocp_profile).

  python scripts/bench_collision_costs.py [--pairs 1 8 20 64] [--batch 256] [--horizon 200] [--steps 40] [--warmup 5]

Sets of up to 8 rows (N <= 5) run on today's default path -- from the second pair on the one-lane-per-node k_calc_qp -- and, with
AGX_COST_WIDE=1, on the wide path; the script runs N = 5 both ways.
"""
from __future__ import annotations

import argparse
import json
import os
import pathlib
import sys
import time

import numpy as np

ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

from agimus_controller_amd import _abi, backend, workloads  # noqa: E402
from agimus_controller_amd.factory import robot_tables as rt  # noqa: E402

CAPSULES = workloads.PANDA_LINK_CAPSULES
SELF_PAIRS = workloads.PANDA_SELF_COLLISION_PAIRS


def make_problem(n_pairs, T):
    n_obs = max(0, -(-(n_pairs - 1 - len(SELF_PAIRS)) // len(CAPSULES))) if n_pairs > 1 else 0
    table = rt.panda_collision_table(0.1, obstacle_xyz=(0.27, 0.22, 0.70), obstacle_radius=0.06, obstacle_length=0.0,
                                     obstacles=workloads.random_obstacles(n_obs))
    tcp = table.frame_id("panda_hand_tcp")
    running, terminal = workloads.goal_reaching_rows(tcp)
    pairs = [("panda_link7_capsule_0", "obstacle")]
    if n_pairs > 1:
        pairs += SELF_PAIRS + [(c, f"ob{i}") for i in range(n_obs) for c in CAPSULES]
    pc = workloads.collision_pair_costs(table, pairs[:n_pairs], _abi.ACT_QUAD_EXP, 0.05, 0.1)
    po = _abi.PackedOcp(7, [0.01] * T, list(running) + pc, list(terminal) + pc, termination_tolerance=1e-3)
    return table, tcp, po


def run(n_pairs, B, T, steps, warmup, wide):
    table, tcp, po = make_problem(n_pairs, T)
    before = os.environ.get("AGX_COST_WIDE")
    if wide is None:
        os.environ.pop("AGX_COST_WIDE", None)
    else:
        os.environ["AGX_COST_WIDE"] = "1" if wide else "0"
    try:
        hip = backend.HipOcp(table, po, B)  # the switch is read when the handle is created
    finally:
        if before is None:
            os.environ.pop("AGX_COST_WIDE", None)
        else:
            os.environ["AGX_COST_WIDE"] = before
    on_wide_path = hip.cost_wide
    q0, amp, puls, scale, t0 = workloads.sine_batch_params(B, lower=table.lower_position_limit, upper=table.upper_position_limit)
    w = workloads.SINE_WEIGHTS
    hip.sine_trajectory(warmup + steps + T + 2, 0.01, q0, amp, puls, scale, t0, w["w_q"], w["w_qdot"], w["w_effort"], w["w_pose"], tcp)
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
    hip.profile(True)
    for k in range(warmup + steps, warmup + steps + 2):
        hip.mpc_step(k, 10, first=False)
    hip.sync()
    ms, cnt = hip.profile(False)
    out = {"pairs": n_pairs, "path": "wide" if on_wide_path else "default", "batch": B, "horizon": T, "steps": steps,
           "steps_per_s": steps / elapsed, "instance_steps_per_s": B * steps / elapsed, "ms_per_step": 1e3 * elapsed / steps,
           "mean_sqp_iter": float(np.mean(iters)), "derivative_pass_ms": hip.time_kernel(0, 20),
           "profile_trial_pass_running_ms": ms[0] / cnt[0] if cnt[0] else None}
    if on_wide_path:
        out["k_cost_pairs_ms"] = hip.time_kernel(9, 20)
    hip.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, nargs="+", default=[1, 8, 20, 64])
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--horizon", type=int, default=200)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()
    for n in args.pairs:
        print(json.dumps(run(n, args.batch, args.horizon, args.steps, args.warmup, None)), flush=True)
    for wide in (False, True):  # the 5-pair problem on today's default (one-lane k_calc_qp) and on the wide path
        print(json.dumps(run(5, args.batch, args.horizon, args.steps, args.warmup, wide)), flush=True)


if __name__ == "__main__":
    main()
