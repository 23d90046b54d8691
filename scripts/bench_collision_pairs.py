"""MPC steps / s on the device with many collision-pair constraints per node (wide constraint sets).

The problem is the Panda of `bench.py --workload collision` (sine_wave_configuration_space references, collision-avoidance
costs with one distance cost row, ADMM with max_qp_iters 100, quorum 0.985) with N collision-pair constraints (distance >= 1 cm)
instead of its one: the link-7 capsule / sphere pair of the workload, then the five link capsules against further obstacles
(capsules, spheres, boxes in turn) and four self-collision pairs.  One JSON line per N: batch steps / s and instance steps / s
(the "MPC steps/s" of bench.py).

  python scripts/bench_collision_pairs.py [--pairs 1 8 20 64] [--batch 256] [--horizon 200] [--steps 40] [--warmup 5]

N = 1 is the workload of bench.py itself (fixed constraint layout); AGX_CON_WIDE=1 in the environment puts it on the wide one.
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

CAPSULES = workloads.PANDA_LINK_CAPSULES
SELF_PAIRS = workloads.PANDA_SELF_COLLISION_PAIRS


def make_problem(n_pairs, T):
    n_obs = max(0, -(-(n_pairs - 1 - len(SELF_PAIRS)) // len(CAPSULES))) if n_pairs > 1 else 0
    table = rt.panda_collision_table(0.1, obstacle_xyz=(0.27, 0.22, 0.70), obstacle_radius=0.06, obstacle_length=0.0,
                                     obstacles=workloads.random_obstacles(n_obs))
    tcp = table.frame_id("panda_hand_tcp")
    running, terminal = workloads.collision_avoidance_rows(table, tcp, alpha=1e-4)
    pairs = [("panda_link7_capsule_0", "obstacle")]
    if n_pairs > 1:
        pairs += SELF_PAIRS + [(c, f"ob{i}") for i in range(n_obs) for c in CAPSULES]
    pairs = pairs[:n_pairs]
    con = workloads.collision_pair_constraints(table, pairs, 0.01)
    po = _abi.PackedOcp(7, [0.01] * T, running, terminal, termination_tolerance=1e-3, max_qp_iters=100, running_constraints=con)
    return table, tcp, po


def run(n_pairs, B, T, steps, warmup, quorum):
    table, tcp, po = make_problem(n_pairs, T)
    hip = backend.HipOcp(table, po, B)
    if quorum < 1.0:
        hip.set_quorum(quorum, quorum)
    q0, amp, puls, scale, t0 = workloads.sine_batch_params(B, lower=table.lower_position_limit, upper=table.upper_position_limit)
    w = workloads.SINE_WEIGHTS
    hip.sine_trajectory(warmup + steps + T + 2, 0.01, q0, amp, puls, scale, t0, w["w_q"], w["w_qdot"], w["w_effort"], w["w_pose"], tcp)
    iters, qp = [], []
    for k in range(warmup):
        hip.mpc_step(k, 10, first=(k == 0))
        hip.download_first(copy=False)
    hip.sync()
    t_start = time.perf_counter()
    for k in range(warmup, warmup + steps):
        hip.mpc_step(k, 10, first=False)
        st = hip.download_first(copy=False)[3]
        iters.append(float(st["iter"].mean()))
        qp.append(float(st["qp_iters"].mean()))
    hip.sync()
    elapsed = time.perf_counter() - t_start
    hip.close()
    return {"pairs": n_pairs, "batch": B, "horizon": T, "steps": steps, "quorum": quorum, "steps_per_s": steps / elapsed, "instance_steps_per_s": B * steps / elapsed,
            "ms_per_step": 1e3 * elapsed / steps, "mean_sqp_iter": float(np.mean(iters)), "mean_qp_iters_last_iter": float(np.mean(qp))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, nargs="+", default=[1, 8, 20, 64])
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--horizon", type=int, default=200)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--quorum", type=float, default=0.985, help="batch quorum (as bench.py reports the collision workload)")
    args = ap.parse_args()
    for n in args.pairs:
        print(json.dumps(run(n, args.batch, args.horizon, args.steps, args.warmup, args.quorum)), flush=True)


if __name__ == "__main__":
    main()
