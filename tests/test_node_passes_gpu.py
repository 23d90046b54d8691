"""The node-parallel passes between the sweeps: for the 7-joint capacity the node shares of the KKT
residual come from k_node_kkt_ahead, which issues every load of a wave ahead of its first wait (AGX_NODE_KKT_WIDE, default on)
instead of k_node_kkt's eight dependent groups of loads.  Only the loads differ: products, row sums and butterflies keep their
operands and order, so everything a solve hands out must be bitwise equal with AGX_NODE_KKT_WIDE=0 and with the default (the
switch is read when a handle is created: both handles live in this process).  One case pins the default to the checker with
the tolerances of tests/test_hip_parity.py."""

import os

import numpy as np
import pytest

from agimus_controller_amd import _abi, workloads
from agimus_controller_amd.factory import robot_tables as rt

pytestmark = pytest.mark.gpu

DT = 0.01
N_STEPS = 4  # the ring origin of the carried tiles is non-zero in steps 2 .. 4


def _handle(backend, wide, table, po, B, n_points, frame):
    old = os.environ.get("AGX_NODE_KKT_WIDE")
    if wide:
        os.environ.pop("AGX_NODE_KKT_WIDE", None)  # the default
    else:
        os.environ["AGX_NODE_KKT_WIDE"] = "0"
    try:
        h = backend.HipOcp(table, po, B)
    finally:
        if old is None:
            os.environ.pop("AGX_NODE_KKT_WIDE", None)
        else:
            os.environ["AGX_NODE_KKT_WIDE"] = old
    nv = table.nv
    q0, amp, puls, scale, t0 = workloads.sine_batch_params(B, nv=nv, seed0=1234, q0=(None if nv == 7 else np.zeros(nv)),
                                                           lower=table.lower_position_limit, upper=table.upper_position_limit)
    w = workloads.SINE_WEIGHTS
    h.sine_trajectory(n_points, DT, q0, amp, puls, scale, t0, w["w_q"], w["w_qdot"], w["w_effort"], w["w_pose"], frame)
    return h


def _run(backend, wide, table, po, B, frame, max_iters):
    """N_STEPS MPC steps on the resident sine trajectory; after the first and the last one also the direction kernels at the
    resident point.  Returns [(xs, us, K, status)] per step and [(du, kkt)]."""
    h = _handle(backend, wide, table, po, B, N_STEPS + po.horizon + 4, frame)
    steps, dirs = [], []
    for k in range(N_STEPS):
        h.mpc_step(k, max_iters[k], first=1 if k == 0 else 0)
        xs, us, K, st = h.download()
        steps.append((xs, us, K, np.array(st)))
        if k in (0, N_STEPS - 1):
            _, _, _, du, kkt = h.direction()
            dirs.append((du, kkt))
    h.close()
    return steps, dirs


def _assert_bitwise(table, po, B, frame, hip_backend, max_iters=(10,) * N_STEPS):
    wide, dwide = _run(hip_backend, True, table, po, B, frame, max_iters)
    narrow, dnarrow = _run(hip_backend, False, table, po, B, frame, max_iters)
    for k, ((du_w, kkt_w), (du_n, kkt_n)) in enumerate(zip(dwide, dnarrow)):
        assert np.all(np.isfinite(du_w)) and np.all(np.isfinite(kkt_w))
        assert np.array_equal(du_w, du_n), f"direction {k}: du differs (max |diff| {np.abs(du_w - du_n).max():.3e})"
        assert np.array_equal(kkt_w, kkt_n), f"direction {k}: kkt differs ({kkt_w} / {kkt_n})"
    for k, (rw, rn) in enumerate(zip(wide, narrow)):
        for field in rw[3].dtype.names:
            assert np.array_equal(rw[3][field], rn[3][field], equal_nan=True), f"step {k}: status word {field} differs"
        for name, vw, vn in zip(("xs", "us", "K"), rw[:3], rn[:3]):
            assert np.array_equal(vw, vn), f"step {k}: {name} differs (max |diff| {np.abs(vw - vn).max():.3e})"
    return wide


def _panda(T):
    table = rt.panda_table(0.1)
    tcp = table.frame_id("panda_hand_tcp")
    running, terminal = workloads.goal_reaching_rows(tcp)
    return table, tcp, _abi.PackedOcp(7, [DT] * T, running, terminal, termination_tolerance=1e-3, max_qp_iters=100)


def test_one_partly_filled_workgroup(hip_backend):
    """B = 3, T = 4: 15 nodes, first-node and terminal branches inside one wave, the last wave partly filled."""
    table, tcp, po = _panda(4)
    _assert_bitwise(table, po, 3, tcp, hip_backend)


def test_five_joints_padded_to_seven(hip_backend):
    """B = 5, T = 9, a 5-joint chain in the 7-joint capacity: the lanes l8 >= nv, and 50 nodes (not a multiple of 8)."""
    table = rt.chain_table(5, seed=25)
    frame = len(table.frame_names) - 1
    running, terminal = workloads.goal_reaching_rows(frame)
    po = _abi.PackedOcp(5, [DT] * 9, running, terminal, termination_tolerance=1e-3, max_qp_iters=100)
    _assert_bitwise(table, po, 5, frame, hip_backend)


def test_waves_of_finished_instances(hip_backend):
    """B = 40, T = 7 (one instance = one wave of 8 nodes), max_iter = 1 on every second step: where instances of one step
    finish after different numbers of iterations, the waves of the finished ones leave early next to waves that work."""
    table, tcp, po = _panda(7)
    runs = _assert_bitwise(table, po, 40, tcp, hip_backend, max_iters=(10, 1, 10, 1))
    assert any(len(np.unique(r[3]["iter"])) > 1 for r in runs), "no step with finished instances next to working ones"


def test_default_against_the_checker(hip_backend, panda, monkeypatch):
    """The default build alone against the oracle: direction kernels at a fixed point and a full solve, tolerances of
    tests/test_hip_parity.py (test_direction_kernels_against_oracle, test_full_solve_matches_oracle)."""
    from oracle.oracle import Oracle

    monkeypatch.delenv("AGX_NODE_KKT_WIDE", raising=False)
    rel = lambda a, b: float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))  # noqa: E731
    tcp = panda.frame_id("panda_hand_tcp")
    B, T = 3, 13  # 42 nodes: five full waves and a wave of two nodes
    po, ref, x0, xs, us = workloads.random_goal_problem(panda, T, 0.01, B, seed=6, frame=tcp)
    h, o = hip_backend.HipOcp(panda, po, B), Oracle(panda, po, B)
    xs[:, 0] = x0
    h.set_refs(ref)
    h.upload_warmstart(xs, us)
    K, k, dx, du, kkt = h.direction()
    Ko, ko, dxo, duo, kkto = o.direction(o.calc_diff(ref, None, xs, us))
    assert rel(dx, dxo) < 1e-9 and rel(du, duo) < 1e-9
    assert rel(K, Ko) < 1e-8
    np.testing.assert_allclose(kkt, kkto, rtol=1e-7)
    xs_h, us_h, K_h, st_h = h.solve(x0, xs, us, 12)
    xs_o, us_o, K_o, st_o = o.solve(ref, None, x0, xs, us, 12, nthreads=8)
    np.testing.assert_array_equal(st_h["iter"], st_o["iter"])
    np.testing.assert_array_equal(st_h["solved"], st_o["solved"])
    assert rel(xs_h, xs_o) < 1e-9 and rel(us_h, us_o) < 1e-9
    assert rel(K_h, K_o) < 1e-7
    np.testing.assert_allclose(st_h["kkt"], st_o["kkt"], rtol=1e-6, atol=1e-12)
    np.testing.assert_allclose(st_h["cost"], st_o["cost"], rtol=1e-10)
    h.close()
