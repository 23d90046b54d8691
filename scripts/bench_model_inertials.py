"""What per-instance controller inertials cost (HipOcp.set_model_inertials), on one handle in one process:

* per launch: the eight-lane derivative pass over the running nodes (agx_ocp_time_kernel(3): k_calc_qp_lj, `--launches`
  back-to-back launches between two events after a warm-up launch) with the inertials cleared, with the nominal table's own
  inertials uploaded for every instance, and with seeded +-10 % tables; `--repeats` times, the three in turn, so that each
  samples the same stretch of time;
* MPC steps / s of the resident sine loop (mpc_step(k, 10, first=0) on the own prediction) without and with them.

  python scripts/bench_model_inertials.py [--batch 1024] [--horizon 100] [--steps 100] [--warmup 10]
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

MODES = ("cleared", "nominal_uploaded", "perturbed")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--horizon", type=int, default=100)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    args = ap.parse_args()
    B, T = args.batch, args.horizon
    table = rt.panda_table(0.1)
    tcp = table.frame_id("panda_hand_tcp")
    po = _abi.PackedOcp(7, [0.01] * T, *workloads.goal_reaching_rows(tcp))
    hip = backend.HipOcp(table, po, B)
    q0, amp, puls, scale, t0 = workloads.sine_batch_params(B, lower=table.lower_position_limit, upper=table.upper_position_limit)
    w = workloads.SINE_WEIGHTS
    n_points = 2 * (args.warmup + args.steps) + T + 4
    hip.sine_trajectory(n_points, 0.01, q0, amp, puls, scale, t0, w["w_q"], w["w_qdot"], w["w_effort"], w["w_pose"], tcp)
    inertials = {"nominal_uploaded": workloads.stack_inertials([table] * B),
                 "perturbed": workloads.stack_inertials(workloads.plant_tables(table, B, seed=1, rel=0.1))}

    def select(mode):
        if mode == "cleared":
            hip.clear_model_inertials()
        else:
            hip.set_model_inertials(*inertials[mode])

    hip.mpc_step(0, 10, first=True)
    ms = {m: [] for m in MODES}
    for _ in range(args.repeats):
        for m in MODES:
            select(m)
            ms[m].append(hip.time_kernel(3, args.launches))
    base = np.array(ms["cleared"])
    for m in MODES:
        t = np.array(ms[m])
        print(json.dumps({"measure": "k_calc_qp_lj per launch", "model_inertials": m, "batch": B, "horizon": T, "ms_mean": float(t.mean()),
                          "ms_min": float(t.min()), "ms_max": float(t.max()), "ms_repeats": [float(v) for v in t],
                          "ratio_to_cleared_mean": float(t.mean() / base.mean()), "launches_per_repeat": args.launches}), flush=True)
    k = 1
    for m in ("cleared", "perturbed", "cleared", "perturbed"):
        select(m)
        for _ in range(args.warmup if k == 1 else 2):
            hip.mpc_step(k, 10, first=0)
            k += 1
        hip.sync()
        n = args.steps // 2
        t_start = time.perf_counter()
        for _ in range(n):
            hip.mpc_step(k, 10, first=0)
            k += 1
        hip.sync()
        rate = n / (time.perf_counter() - t_start)
        st = hip.download(want_K=False)[3]
        print(json.dumps({"measure": "resident sine loop", "model_inertials": m, "batch": B, "horizon": T, "steps": n, "steps_per_s": rate,
                          "instance_steps_per_s": B * rate, "mean_iter": float(np.mean(st["iter"])), "finite": bool(np.all(np.isfinite(st["cost"])))}),
              flush=True)
    hip.close()


if __name__ == "__main__":
    main()
