"""What per-instance obstacle placements (agx_ocp_set_obstacle_placements) cost: MPC steps / s and per-launch kernel times with
and without the table, all legs in one process.

Panda, B = 256, T = 200, sine_wave_configuration_space references, four workloads:
  row      the cost rows of `bench.py --workload collision` (one QuadExp distance row: eight-lane K1 with COLL)
  soft8    8 soft pairs   (scripts/bench_collision_costs.py: wide cost set, k_cost_pairs)
  soft64   64 soft pairs
  hard20   20 pair constraints at quorum 0.985 (scripts/bench_collision_pairs.py: wide constraint set, k_con_eval_pairs)
and three legs per workload:
  (a) no table, three repeats: their spread is the yardstick;
  (b) the table filled with the model's own placements for every obstacle of the workload: the same problems on the
      instantiations that read the table -- the iteration counts of every step must equal those of (a);
  (c) seeded per-instance placements (`workloads.obstacle_placements`, 0.05 m, 0.3 rad): other problems, reported only.
One JSON line per leg: instance steps / s, mean SQP iterations, the per-launch time of the derivative pass (kernel 0 of
agx_ocp_time_kernel: K1, with k_cost_pairs on a wide cost set) and of k_cost_pairs alone (kernel 9) where there is one; then the
host time of one set_obstacle_placements call.  (agx_ocp_time_kernel has no entry for the constraint evaluation: hard20 shows
its cost in the step rate only.)

  python scripts/bench_obstacle_placements.py [--batch 256] [--horizon 200] [--steps 40] [--warmup 5]
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
sys.path.insert(0, str(ROOT / "scripts"))

import bench_collision_costs as soft  # noqa: E402
import bench_collision_pairs as hard  # noqa: E402
from agimus_controller_amd import _abi, backend, workloads  # noqa: E402
from agimus_controller_amd.factory import robot_tables as rt  # noqa: E402


def make_problem(workload, T):
    """(table, tool frame, problem, quorum)"""
    if workload == "row":
        table = rt.panda_collision_table(0.1, obstacle_xyz=(0.27, 0.22, 0.70), obstacle_radius=0.06, obstacle_length=0.0)
        tcp = table.frame_id("panda_hand_tcp")
        running, terminal = workloads.collision_avoidance_rows(table, tcp, alpha=1e-4)
        return table, tcp, _abi.PackedOcp(7, [0.01] * T, running, terminal, termination_tolerance=1e-3), 1.0
    if workload.startswith("soft"):
        return soft.make_problem(int(workload[4:]), T) + (1.0,)
    return hard.make_problem(int(workload[4:]), T) + (0.985,)


def obstacles_of(table):
    """Every world-fixed geometry frame of the table."""
    rad = np.zeros(len(table.frame_names)) if table.frame_radius is None else np.asarray(table.frame_radius)
    box = np.zeros((len(table.frame_names), 3)) if table.frame_box is None else np.asarray(table.frame_box).reshape(-1, 3)
    return [f for f in range(len(table.frame_names)) if table.frame_parent[f] < 0 and (rad[f] > 0.0 or np.any(box[f] > 0.0))]


def run(workload, leg, B, T, steps, warmup):
    table, tcp, po, quorum = make_problem(workload, T)
    hip = backend.HipOcp(table, po, B)
    if quorum < 1.0:
        hip.set_quorum(quorum, quorum)
    q0, amp, puls, scale, t0 = workloads.sine_batch_params(B, lower=table.lower_position_limit, upper=table.upper_position_limit)
    w = workloads.SINE_WEIGHTS
    hip.sine_trajectory(warmup + steps + T + 2, 0.01, q0, amp, puls, scale, t0, w["w_q"], w["w_qdot"], w["w_effort"], w["w_pose"], tcp)
    frames = obstacles_of(table)
    set_ms = None
    if leg != "a":
        se3 = (workloads.obstacle_placements(table, frames, B, 0, 0.0, 0.0) if leg == "b" else
               workloads.obstacle_placements(table, frames, B, 1, 0.05, 0.3))
        hip.set_obstacle_placements(frames, se3)  # (allocates)
        hip.sync()
        t_set = time.perf_counter()
        for _ in range(5):
            hip.set_obstacle_placements(frames, se3)
        set_ms = 1e3 * (time.perf_counter() - t_set) / 5
    iters = []
    for k in range(warmup):
        hip.mpc_step(k, 10, first=(k == 0))
        iters.append(hip.download_first(copy=False)[3]["iter"].copy())
    hip.sync()
    t_start = time.perf_counter()
    for k in range(warmup, warmup + steps):
        hip.mpc_step(k, 10, first=False)
        iters.append(hip.download_first(copy=False)[3]["iter"].copy())
    hip.sync()
    elapsed = time.perf_counter() - t_start
    out = {"workload": workload, "leg": leg, "batch": B, "horizon": T, "steps": steps, "obstacles": len(frames), "wide_costs": hip.cost_wide,
           "instance_steps_per_s": B * steps / elapsed, "ms_per_step": 1e3 * elapsed / steps,
           "mean_sqp_iter": float(np.mean(iters[warmup:])), "derivative_pass_ms": hip.time_kernel(0, 20)}
    if hip.cost_wide:
        out["k_cost_pairs_ms"] = hip.time_kernel(9, 20)
    if set_ms is not None:
        out["set_obstacle_placements_ms"] = set_ms
        out["table_bytes"] = int(B * len(frames) * 96)
    hip.close()
    return out, np.array(iters)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", nargs="+", default=["row", "soft8", "soft64", "hard20"])
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--horizon", type=int, default=200)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()
    mismatches = []
    for wl in args.workloads:
        base, rates = None, []
        for leg in ("a", "a", "a", "b", "c"):
            out, iters = run(wl, leg, args.batch, args.horizon, args.steps, args.warmup)
            print(json.dumps(out), flush=True)
            if leg == "a":
                rates.append(out["instance_steps_per_s"])
                if base is None:
                    base = iters
                elif not np.array_equal(iters, base):
                    print(json.dumps({"workload": wl, "note": "iteration counts of two (a) repeats differ"}), flush=True)
            elif leg == "b":
                same = bool(np.array_equal(iters, base))
                lo, hi = min(rates), max(rates)
                print(json.dumps({"workload": wl, "a_min": lo, "a_max": hi, "a_spread_pct": 100.0 * (hi - lo) / hi, "b": out["instance_steps_per_s"],
                                  "b_vs_a_mean_pct": 100.0 * (out["instance_steps_per_s"] / float(np.mean(rates)) - 1.0),
                                  "b_within_spread": bool(lo <= out["instance_steps_per_s"] <= hi), "b_same_iteration_counts": same}), flush=True)
                if not same:
                    mismatches.append(wl)
    # asserted after every leg has been reported
    assert not mismatches, f"the table filled with the model's placements changed the iteration counts of {mismatches}"


if __name__ == "__main__":
    main()
