"""Development: MPC step time of the Panda with its real gripper (robot_tables.panda_gripper_table: nv = 9, two prismatic finger
joints; runs at the 16-joint capacity) on the default bench workload shape (sine references, goal-reaching costs).  The loop of
scripts/run_fingers.py, whose model stands in for the fingers with two random revolute joints."""
import argparse, pathlib, sys, time
import numpy as np
ROOT = pathlib.Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
from agimus_controller_amd import _abi, backend, workloads  # noqa: E402
from agimus_controller_amd.factory import robot_tables as rt  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=256)
ap.add_argument("--horizon", type=int, default=50)
ap.add_argument("--steps", type=int, default=50)
a = ap.parse_args()
table = rt.panda_gripper_table()
tcp = table.frame_id("panda_hand_tcp")
B, T, dt = a.batch, a.horizon, 0.01
running, terminal = workloads.goal_reaching_rows(tcp)
po = _abi.PackedOcp(9, [dt] * T, running, terminal)
h = backend.HipOcp(table, po, B)
# the arm as in the 7-joint bench workload; the fingers swing by 1 cm about the middle of their 0 ... 0.04 m stroke
q0, amp, puls, scale, t0 = workloads.sine_batch_params(B, nv=9, seed0=3, q0=np.concatenate([workloads.PANDA_Q0, [0.02, 0.02]]))
amp[:, 7:] = 0.01
q0[:, 7:] = 0.02
w = workloads.SINE_WEIGHTS
h.sine_trajectory(a.steps + 5 + T + 2, dt, q0, amp, puls, scale, t0, w["w_q"], w["w_qdot"], w["w_effort"], w["w_pose"], tcp)
for k in range(5):
    h.mpc_step(k, 10, first=(k == 0))
    h.download_first(copy=False)
h.sync()
lat = []
for k in range(5, 5 + a.steps):
    t1 = time.perf_counter()
    h.mpc_step(k, 10, first=False)
    st = h.download_first(copy=False)[3]
    lat.append((time.perf_counter() - t1) * 1e3)
print(f"panda_gripper nv 9 batch {B} T {T}: median {np.median(lat):.3f} ms per step, {B * 1e3 / np.mean(lat):.0f} steps/s, "
      f"mean iters {st['iter'].mean():.2f}, solved {int(np.sum(st['solved']))} of {B}")
h.close()
