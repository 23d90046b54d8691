"""Streamed resident trajectory against the one-shot resident loop and the host-tile path, in one process.

Workload: Panda, goal-reaching rows (stride 63), B = 1024, T = 100; the samples are the q, dq, ddq arrays of bench.py's
`--workload generic` (workloads.generic_batch_arrays from the q0 of sine_batch_params), computed on the host, with the
SINE_WEIGHTS of the sine workload.  Every leg starts at sample 0 on a handle of its own and runs `--warmup` + `--steps` steps
of mpc_step(k, 10) + download_first, timed between two device synchronisations:

  A  (three times: before, between and after the other legs) the one-shot loop on `generic_trajectory`;
  B  the streamed loop on a ring of capacity 4 (T + 1): each step stream_append of ONE sample per instance -- the last sample
     of the step's own window (`--lead 0`; the solver stream waits for the fill) --, stream_release(k), mpc_step(k);
  B+ the same with the appends `--lead-ahead` samples ahead of the window (a planner that runs ahead);
  C  the host path: the [B][T+1][stride] tile of every step assembled in page-locked memory by worker threads and staged with
     set_refs_async / refs_activate, x0_from_prediction + shift_warmstart + solve_resident (no tile carry).

Also: the device time of one append (transfer + fill of one sample per instance, hipEvents on the copy stream:
time_kernel(10)), the host time the B leg spends inside stream_append / stream_release / mpc_step, whether B's last result
equals A's bit for bit, and both streamed legs once more with `stream_timing` on: hipEvents on the solver stream around every
wait for a fill and on the copy stream around every append, over the timed steps.  One JSON line per leg and a summary line.  Run it under a time limit of its own, e.g.

  timeout -k 10 900 python scripts/bench_stream.py [--batch 1024] [--horizon 100] [--steps 200] [--warmup 20]
"""
from __future__ import annotations

import argparse
import concurrent.futures as cf
import json
import pathlib
import sys
import time

import numpy as np

ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

from agimus_controller_amd import _abi, backend, workloads  # noqa: E402
from agimus_controller_amd.factory import robot_tables as rt  # noqa: E402

MAX_ITER = 10


def problem(T):
    table = rt.panda_table(0.1)
    tcp = table.frame_id("panda_hand_tcp")
    po = _abi.PackedOcp(7, [0.01] * T, *workloads.goal_reaching_rows(tcp), termination_tolerance=1e-3, max_qp_iters=100)
    return table, tcp, po


def one_shot(table, tcp, po, B, samples):
    h = backend.HipOcp(table, po, B)
    w = workloads.SINE_WEIGHTS
    h.generic_trajectory(*samples, w["w_q"], w["w_qdot"], w["w_effort"], w["w_pose"], tcp)
    return h


def leg_resident(h, warmup, steps):
    for k in range(warmup + steps):
        if k == warmup:
            h.sync()
            t0 = time.perf_counter()
        h.mpc_step(k, MAX_ITER, first=(k == 0))
        h.download_first(copy=False)
    h.sync()
    return steps / (time.perf_counter() - t0), h.download_first(copy=True)


def leg_streamed(table, tcp, po, B, samples, warmup, steps, lead, timing=False):
    T = po.horizon
    q, dq, ddq = samples
    h = backend.HipOcp(table, po, B)
    w = workloads.SINE_WEIGHTS
    h.stream_trajectory(4 * (T + 1), T + 1, w["w_q"], w["w_qdot"], w["w_effort"], np.full(6, w["w_pose"]), tcp)
    h.stream_append(q[:, :T + lead], dq[:, :T + lead], ddq[:, :T + lead])
    # what a planner hands over per step: one contiguous [B][1][nv] array per quantity (laid out before the timed region)
    per_step = [np.ascontiguousarray(a.transpose(1, 0, 2))[:, :, None, :] for a in (q, dq, ddq)]
    host = {"stream_append": 0.0, "stream_release": 0.0, "mpc_step": 0.0, "download_first": 0.0}
    for k in range(warmup + steps):
        if k == warmup:
            h.sync()
            host = dict.fromkeys(host, 0.0)
            if timing:
                h.stream_timing(True)
            t0 = time.perf_counter()
        j = k + T + lead  # the sample this step brings
        ta = time.perf_counter()
        h.stream_append(per_step[0][j], per_step[1][j], per_step[2][j])
        tb = time.perf_counter()
        h.stream_release(k)
        tc = time.perf_counter()
        h.mpc_step(k, MAX_ITER, first=(k == 0))
        td = time.perf_counter()
        h.download_first(copy=False)
        te = time.perf_counter()
        for name, dtm in zip(host, (tb - ta, tc - tb, td - tc, te - td)):
            host[name] += dtm
    h.sync()
    rate = steps / (time.perf_counter() - t0)
    events = None
    if timing:  # hipEvents of both streams over the timed steps
        ms, cnt = h.stream_timing(False)
        events = {"solver_stream_wait_ms_per_step": ms[0] / steps, "joins": cnt[0], "copy_stream_append_ms_per_piece": ms[1] / max(cnt[1], 1),
                  "appended_pieces": cnt[1]}
    last = h.download_first(copy=True)
    append_ms = [h.time_kernel(10, 50) for _ in range(3)]  # one sample per instance: the last append
    h.close()
    return rate, last, {k: v / steps * 1e3 for k, v in host.items()}, append_ms, events


def leg_host_tiles(table, tcp, po, B, ha, warmup, steps):
    """`ha`: a one-shot handle on the same samples; its tiles and points are read back once, outside the timed region."""
    T, n = po.horizon, warmup + steps + po.horizon + 3
    run = np.stack([ha.traj_tile(k) for k in range(n)], axis=1)
    term = np.stack([ha.traj_tile(k, terminal=True) for k in range(n)], axis=1)
    pts = [ha.traj_point(t) for t in range(T + 1)]
    xs0 = np.stack([np.concatenate(p[:2], axis=1) for p in pts], axis=1)
    us0 = np.stack([p[3] for p in pts[:T]], axis=1)
    h = backend.HipOcp(table, po, B)
    n_workers = 8
    pool = cf.ThreadPoolExecutor(n_workers)
    tiles = [backend.pinned_array((B, T + 1, po.stride)) for _ in range(3)]
    cuts = np.linspace(0, B, n_workers + 1).astype(int)

    def fill(k, out, lo, hi):
        out[lo:hi, :T] = run[lo:hi, k:k + T]
        out[lo:hi, T] = term[lo:hi, k + T]

    def build(k, out):
        return [pool.submit(fill, k, out, int(lo), int(hi)) for lo, hi in zip(cuts[:-1], cuts[1:]) if hi > lo]

    cf.wait(build(0, tiles[0]))
    h.set_refs_async(tiles[0])
    pending = build(1, tiles[1])
    h.upload_x0(xs0[:, 0])
    h.upload_warmstart(xs0, us0)
    for k in range(warmup + steps):
        if k == warmup:
            h.sync()
            t0 = time.perf_counter()
        h.refs_activate()  # tile k, staged during step k - 1
        cf.wait(pending)
        h.set_refs_async(tiles[(k + 1) % 3])  # travels while step k is solved
        pending = build(k + 2, tiles[(k + 2) % 3])
        if k > 0:
            h.x0_from_prediction()
            h.shift_warmstart()
        h.solve_resident(MAX_ITER)
        h.download_first(copy=False)
    h.sync()
    rate = steps / (time.perf_counter() - t0)
    cf.wait(pending)
    h.refs_wait()
    pool.shutdown()
    nbytes = int(tiles[0].nbytes)
    h.close()
    return rate, nbytes


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--horizon", type=int, default=100)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--lead", type=int, default=0, help="leg B: samples the appends run ahead of the window's last sample")
    ap.add_argument("--lead-ahead", type=int, default=8, help="leg B+: the same for the second streamed leg")
    args = ap.parse_args()
    B, T = args.batch, args.horizon
    assert backend.device_count() > 0, "bench_stream.py needs a HIP device"
    table, tcp, po = problem(T)
    n_points = args.warmup + args.steps + T + 3 + max(args.lead, args.lead_ahead)
    q0 = workloads.sine_batch_params(B, lower=table.lower_position_limit, upper=table.upper_position_limit)[0]
    samples = workloads.generic_batch_arrays(B, n_points, 0.01, seed0=1234, q0=q0)
    base = {"batch": B, "horizon": T, "steps": args.steps, "warmup": args.warmup, "max_iter": MAX_ITER, "unit": "MPC instance-steps/s"}

    def report(leg, rate, **extra):
        print(json.dumps({"leg": leg, **base, "steps_per_s": rate, "value": B * rate, "ms_per_step": 1e3 / rate, **extra}), flush=True)

    a_rates, a_last = [], None

    def leg_a(name):
        nonlocal a_last
        h = one_shot(table, tcp, po, B, samples)
        rate, a_last = leg_resident(h, args.warmup, args.steps)
        a_rates.append(rate)
        report(name, rate, what="one-shot resident loop (generic_trajectory)")
        return h

    leg_a("A1").close()
    rate_b, last_b, host_b, app_b, _ = leg_streamed(table, tcp, po, B, samples, args.warmup, args.steps, args.lead)
    equal = all(np.array_equal(x, y) for x, y in zip(last_b[:3], a_last[:3]))
    report("B", rate_b, what=f"streamed loop, ring of {4 * (T + 1)}, one appended sample per step, lead {args.lead}", host_ms_per_step=host_b,
           append_device_ms=app_b, append_bytes=int(B * 3 * 7 * 8), last_result_equals_A=equal)
    leg_a("A2").close()
    rate_b2, last_b2, host_b2, app_b2, _ = leg_streamed(table, tcp, po, B, samples, args.warmup, args.steps, args.lead_ahead)
    report("B+", rate_b2, what=f"streamed loop, appends {args.lead_ahead} samples ahead of the window", host_ms_per_step=host_b2,
           append_device_ms=app_b2, last_result_equals_A=all(np.array_equal(x, y) for x, y in zip(last_b2[:3], a_last[:3])))
    # the two streamed legs once more with events on both streams (legs of their own: the events are not in the figures above)
    for name, lead in (("B events", args.lead), ("B+ events", args.lead_ahead)):
        r, _, host_e, _, ev = leg_streamed(table, tcp, po, B, samples, args.warmup, args.steps, lead, timing=True)
        report(name, r, what=f"streamed loop, lead {lead}, with stream_timing on", host_ms_per_step=host_e, events=ev)
    ha = leg_a("A3")
    rate_c, nbytes = leg_host_tiles(table, tcp, po, B, ha, args.warmup, args.steps)
    ha.close()
    report("C", rate_c, what="host tiles: set_refs_async / refs_activate + shift + solve_resident (8 assembling threads)", h2d_bytes_per_step=nbytes)
    a = np.array(a_rates)
    spread = float(a.max() - a.min())
    print(json.dumps({"summary": True, **base, "A_steps_per_s": [float(v) for v in a], "A_mean": float(a.mean()), "A_spread": spread,
                      "B_steps_per_s": rate_b, "B_minus_A_mean": rate_b - float(a.mean()), "B_within_A_spread": bool(rate_b >= a.mean() - spread),
                      "B_plus_steps_per_s": rate_b2, "C_steps_per_s": rate_c, "append_device_ms": float(np.mean(app_b))}), flush=True)


if __name__ == "__main__":
    main()
