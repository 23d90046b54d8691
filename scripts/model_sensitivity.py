"""The reference's model-sensitivity study (agimus_controller_examples/main/model_sensibility/evaluate_model_sensibility.py) on the
device: how far the next state of the Euler node moves when a link's inertia, centre of mass or mass is off.

For each of the five measured Panda samples (x0, u0) of state_and_control_expe_data.yaml it prints the singular values of the
2 nv x 10 nv sensitivity matrix and the columns (link parameters) that dominate the first right singular vector.  All five
samples are one launch (`HipOcp.model_sensitivity`); no plotting.

  python scripts/model_sensitivity.py [--points tests/golden/state_and_control_expe_data.yaml] [--dt 0.01] [--delta 0.01]
"""
from __future__ import annotations

import argparse
import pathlib
import sys

import numpy as np

ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

from agimus_controller_amd import _abi, backend, workloads  # noqa: E402
from agimus_controller_amd.factory import robot_tables as rt  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", default=str(ROOT / "tests" / "golden" / "state_and_control_expe_data.yaml"))
    ap.add_argument("--dt", type=float, default=0.01)
    ap.add_argument("--delta", type=float, default=0.01, help="delta_inertia = delta_com = delta_mass, as upstream")
    args = ap.parse_args()
    x, u = workloads.load_state_control_points(args.points)
    table = rt.panda_table(0.1)  # armature 0.1 on every joint, as the script sets it
    po = _abi.PackedOcp(7, [args.dt], *workloads.regulation_rows())
    hip = backend.HipOcp(table, po, 1)
    S = hip.model_sensitivity(x, u, args.dt, args.delta, args.delta, args.delta)
    hip.close()
    cols = workloads.sensitivity_columns(table.nv)
    np.set_printoptions(precision=4, linewidth=160, suppress=False)
    for k in range(S.shape[0]):
        _, s, vh = np.linalg.svd(S[k])
        top = np.argsort(-np.abs(vh[0]))[:5]
        print(f"point_{k + 1}: singular values {s}")
        print("   first right singular vector, largest entries:", ", ".join(f"{cols[c]} {abs(vh[0, c]):.3f}" for c in top))


if __name__ == "__main__":
    main()
