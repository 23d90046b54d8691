"""What a clearance report (agx_ocp_clearance / HipOcp.clearance) costs.

Two models:
  panda      the Panda collision table of scripts/bench_collision_costs.py (five link capsules, `obstacle`, eight more obstacles:
             capsules, spheres and boxes), B = 1024, T = 100, the first 1 / 10 / 44 of its 44 pairs;
  humanoid   the 30-joint humanoid with a capsule on eight links and five sphere obstacles, B = 512, T = 50, 44 pairs
and for each pair count four calls: distances alone or with the witness points, at the resident iterate (q = None, T + 1 samples)
or at T + 1 given configurations.  One JSON line per call: `call_ms` is the host clock around calls that end in the call's own
wait for the stream -- upload of the pair table (and of q), the kernel, the download of the results into pageable memory --
and `out_mb` the size of what comes back, which is most of that time.  The Panda handles carry the same pairs as cost rows of a
wide cost set, so `k_cost_pairs_ms` (agx_ocp_time_kernel 9, device events, one launch over B (T + 1) nodes) stands next to it as a
yardstick of a kernel that evaluates the same distances.

The kernel's own time comes from a kernel trace, in a run of its own, one configuration at a time so that the per-kernel
statistics belong to it:

  rocprofv3 --kernel-trace --stats -d OUT -- python scripts/bench_clearance.py --only panda:44:0:iterate --reps 20

(--only MODEL:PAIRS:WITNESS:SOURCE; the k_clearance and k_cost_pairs rows of the statistics are the two figures.)

  python scripts/bench_clearance.py [--reps 5] [--models panda humanoid]
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
sys.path.insert(0, str(ROOT / "scripts"))

import bench_collision_costs as soft  # noqa: E402
from agimus_controller_amd import _abi, backend, workloads  # noqa: E402
from agimus_controller_amd.factory import robot_tables as rt  # noqa: E402

SHAPES = {"panda": (1024, 100, (1, 10, 44)), "humanoid": (512, 50, (44,))}
HUMANOID_LINKS = ["torso_roll", "head_yaw", "l_elbow", "r_elbow", "l_wrist_roll", "r_wrist_roll", "l_knee", "r_knee"]


def panda_handle(n_pairs, B, T):
    """The handle of bench_collision_costs with the n pairs as the cost rows of a wide cost set, and the pairs."""
    table, _, po = soft.make_problem(n_pairs, T)
    before = os.environ.get("AGX_COST_WIDE")
    os.environ["AGX_COST_WIDE"] = "1"  # (one pair is a wide set only when asked for; read when the handle is created)
    try:
        hip = backend.HipOcp(table, po, B)
    finally:
        if before is None:
            os.environ.pop("AGX_COST_WIDE", None)
        else:
            os.environ["AGX_COST_WIDE"] = before
    rows = po.running[len(po.running) - n_pairs:]
    return table, hip, [(r.frame, r.frame_b) for r in rows]


def humanoid_handle(n_pairs, B, T):
    table = rt.humanoid30_table()
    for name in HUMANOID_LINKS:
        table = table.with_geometry(f"{name}_capsule", table.joint_names.index(name), rt.se3(None, [0.0, 0.0, -0.05]), 0.05, 0.08)
    rng = np.random.default_rng(3)
    for i in range(5):
        table = table.with_geometry(f"ob{i}", -1, rt.se3(None, [rng.uniform(0.3, 0.7), rng.uniform(-0.5, 0.5), rng.uniform(0.3, 1.5)]), rng.uniform(0.04, 0.1))
    caps = [f"{name}_capsule" for name in HUMANOID_LINKS]
    pairs = [(caps[2], caps[3]), (caps[4], caps[5]), (caps[4], caps[7]), (caps[1], caps[4])] + [(c, f"ob{i}") for i in range(5) for c in caps]
    running, terminal = workloads.regulation_rows()
    hip = backend.HipOcp(table, _abi.PackedOcp(table.nv, [0.01] * T, list(running), list(terminal)), B)
    return table, hip, [(table.frame_id(a), table.frame_id(b)) for a, b in pairs[:n_pairs]]


def run(model, n_pairs, witness, source, reps):
    B, T, _ = SHAPES[model]
    table, hip, pairs = (panda_handle if model == "panda" else humanoid_handle)(n_pairs, B, T)
    nv = table.nv
    rng = np.random.default_rng(1)
    lo, up = np.asarray(table.lower_position_limit, dtype=float), np.asarray(table.upper_position_limit, dtype=float)
    q = rng.uniform(0.5 * lo, 0.5 * up, (B, T + 1, nv))
    hip.upload_warmstart(np.concatenate([q, np.zeros_like(q)], -1), np.zeros((B, T, nv)))
    kw = dict(witness=bool(witness), q=None if source == "iterate" else q)
    for _ in range(2):  # the first call allocates the handle's block
        hip.clearance(pairs, **kw)
    hip.sync()
    t0 = time.perf_counter()
    for _ in range(reps):
        hip.clearance(pairs, **kw)
    call_ms = 1e3 * (time.perf_counter() - t0) / reps
    items = B * (T + 1) * n_pairs
    out = {"model": model, "batch": B, "horizon": T, "pairs": n_pairs, "witness": bool(witness), "source": source, "reps": reps,
           "call_ms": call_ms, "out_mb": items * 8 * (10 if witness else 1) / 1e6}
    if hip.cost_wide:
        out["k_cost_pairs_ms"] = hip.time_kernel(9, 20)
    hip.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--models", nargs="+", default=["panda", "humanoid"], choices=list(SHAPES))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--only", help="MODEL:PAIRS:WITNESS:SOURCE, e.g. panda:44:0:iterate -- one configuration (for a kernel trace)")
    args = ap.parse_args()
    assert backend.device_count() > 0, "bench_clearance.py needs a HIP device"
    if args.only:
        model, n, w, source = args.only.split(":")
        assert source in ("iterate", "q")
        print(json.dumps(run(model, int(n), int(w), source, args.reps)), flush=True)
        return
    for model in args.models:
        for n in SHAPES[model][2]:
            for witness in (0, 1):
                for source in ("iterate", "q"):
                    print(json.dumps(run(model, n, witness, source, args.reps)), flush=True)


if __name__ == "__main__":
    main()
