"""ResidualModelControlGrav and ResidualModelFrameVelocity cost rows on models of 8 to 32 joints: k_general_rows_wg adds the rows
into the tiles of the workgroup-per-node derivative pass and k_node_kkt_big_gen forms the KKT shares (csrc/agx_general_rows.hpp).
Row set: tests/test_general_rows.py::general_problem as it is.  References: the CPU checker, and for models with prismatic joints
a numpy reference for the two residuals on top of tests/joint_ref.py, pinned to the checker below."""
import numpy as np
import pytest

import joint_ref as jr
import test_general_rows as general
import test_model_sizes as sizes
from agimus_controller_amd import _abi, workloads
from agimus_controller_amd.factory import robot_tables as rt
from oracle.oracle import Oracle

TOL16 = 1e-10  # tests/test_item_costs_gpu.py: the tile tolerance of the large capacities
_jr_residual = jr.residual


def general_residual(t, kind, frame, frame_b, rref, x, u):
    """jr.residual plus r = u - rnea(q, 0, 0) and the frame twist sum_{j on the path} S_j qd_j in the three reference frames."""
    nv = t.nv
    x = np.asarray(x)
    q, qd = x[..., :nv], x[..., nv:]
    if kind == _abi.RES_CONTROL_GRAV:
        return np.asarray(u) - jr.rnea(t, q, 0.0 * q, 0.0 * q)
    if kind == _abi.RES_FRAME_VELOCITY:
        _, _, S = jr.fk(t, q)
        v0 = np.zeros(q.shape[:-1] + (6,)) + 0.0 * q[..., :1]
        j = int(t.frame_parent[frame])
        while j >= 0:
            v0 = v0 + S[j] * qd[..., j, None]
            j = int(t.parent[j])
        RF, pF = jr.frame_placement(t, frame, q)
        lin, ang = v0[..., :3] + np.cross(v0[..., 3:], pF), v0[..., 3:]
        if frame_b == 1:
            Rt = np.swapaxes(RF, -1, -2)
            lin, ang = jr._mv(Rt, lin), jr._mv(Rt, ang)
        vel = v0 if frame_b == 0 else np.concatenate([lin, ang], -1)
        return vel - np.asarray(rref, dtype=float)[..., :6]
    return _jr_residual(t, kind, frame, frame_b, rref, x, u)


def _close(got, want, nv, what, tol=TOL16):
    """every block of the canonical tile to tol x its largest entry"""
    for field, s in _abi.tile_slices(nv).items():
        err, scale = float(np.abs(got[..., s] - want[..., s]).max()), float(np.abs(want[..., s]).max())
        print(f"{what} {field}: err {err:.3e} scale {scale:.3e}")
        assert err <= tol * scale + 1e-13, (what, field)


def _cross_blocks(tiles, nv):
    """(Lxu, Lxx[q, v]) of canonical tiles"""
    sl = _abi.tile_slices(nv)
    Lxx = tiles[..., sl["Lxx"]].reshape(tiles.shape[:-1] + (2 * nv, 2 * nv))
    return tiles[..., sl["Lxu"]], Lxx[..., :nv, nv:]


# ------------------------------------------------------------------------------------------------------------------ CPU
@pytest.mark.parametrize("ref_frame", [0, 1, 2])
def test_numpy_reference_is_the_checker_on_a_revolute_tree(monkeypatch, ref_frame):
    monkeypatch.setattr(jr, "residual", general_residual)
    table = rt.tree_table(9, seed=3)
    po, ref, x0, xs, us = general.general_problem(table, 4, 2, seed=7, ref_frame=ref_frame)
    want = Oracle(table, po, 2).calc_diff(ref, None, xs, us)
    got = jr.calc_diff(table, po, ref, xs, us)
    _close(got, want, 9, f"numpy reference, frame {ref_frame}")
    Lxu, Lqv = _cross_blocks(want, 9)
    assert np.abs(Lxu).max() > 1e-6 and np.abs(Lqv).max() > 1e-6


def test_numpy_reference_on_the_gripper_against_finite_differences(monkeypatch):
    """The Panda with its prismatic fingers: the gradient of the reference's tiles is the central difference of its node cost."""
    monkeypatch.setattr(jr, "residual", general_residual)
    table = rt.panda_gripper_table()
    po, ref, x0, xs, us = general.general_problem(table, 2, 1, seed=9, ref_frame=1)
    sl = _abi.tile_slices(9)
    tile = jr.node_tile(table, po, False, 0.01, xs[0, 0], us[0, 0], ref[0, 0])
    z, h = np.concatenate([xs[0, 0], us[0, 0]]), 1e-6
    cost = lambda zz: jr.node_cost(table, po, False, 0.01, zz[:18], zz[18:], ref[0, 0])  # noqa: E731
    fd = np.array([(cost(z + h * e) - cost(z - h * e)) / (2 * h) for e in np.eye(27)])
    np.testing.assert_allclose(np.concatenate([tile[sl["Lx"]], tile[sl["Lu"]]]), fd, rtol=2e-5, atol=1e-8)
    Lxu, Lqv = _cross_blocks(tile, 9)
    assert np.abs(Lxu).max() > 1e-6 and np.abs(Lqv).max() > 1e-6


def test_workloads_general_rows_is_the_row_set_of_general_problem():
    table = rt.tree_table(9, seed=3)
    po = general.general_problem(table, 2, 1, seed=1, ref_frame=2)[0]
    running, terminal = workloads.general_rows(len(table.frame_names) - 1, ref_frame=2)
    key = lambda rows: [(r.kind, r.frame, r.frame_b, r.name) for r in rows]  # noqa: E731
    assert key(running) == key(po.running) and key(terminal) == key(po.terminal)
    assert [r.kind for r in workloads.general_rows(0, with_placement=False, with_grav=False)[0]] == [_abi.RES_CONTROL, _abi.RES_STATE, _abi.RES_FRAME_VELOCITY]


# ------------------------------------------------------------------------------------------------------------------ GPU
B = 2
MODELS = {"tree9": lambda: rt.tree_table(9, seed=3), "chain12": lambda: rt.chain_table(12, seed=4), "tree16": lambda: rt.tree_table(16, seed=5),
          "humanoid30": rt.humanoid30_table, "chain31": lambda: rt.chain_table(31, seed=6), "chain32": lambda: rt.chain_table(32, seed=8),
          "gripper": rt.panda_gripper_table}


def _problem(name, T, seed, ref_frame=0, with_grav=True):
    """general_problem on the model; at 32 joints without the FramePlacement row (the five-row tile exceeds 256 doubles)."""
    table = MODELS[name]()
    po, ref, x0, xs, us = general.general_problem(table, T, B, seed, ref_frame, with_grav)
    if table.nv == 32:
        keep = [i for i, r in enumerate(po.running) if r.kind != _abi.RES_FRAME_PLACEMENT]
        po4 = _abi.PackedOcp(32, [0.01] * T, [po.running[i] for i in keep], po.terminal)
        ref4 = po4.new_ref_tile(B)
        for k, i in enumerate(keep):
            o_old, o_new, w = po.running_offsets[i], po4.running_offsets[k], po.running[i].width(32)
            ref4[:, :T, o_new:o_new + w] = ref[:, :T, o_old:o_old + w]
        ref4[:, T, :] = 0.0
        wt = sum(r.width(32) for r in po.terminal)
        ref4[:, T, :wt] = ref[:, T, :wt]
        po, ref = po4, ref4
    xs[:, 0] = x0
    return table, po, ref, x0, xs, us


def _reference_tiles(name, table, po, ref, xs, us):
    if name == "gripper":
        return jr.calc_diff(table, po, ref, xs, us)
    return Oracle(table, po, B).calc_diff(ref, None, xs, us)


def _handle(hip_backend, table, po, ref):
    h = hip_backend.HipOcp(table, po, B)
    assert h.general_rows and hip_backend.lib().agx_ocp_general_rows(h._h) == 1
    h.set_refs(ref)
    return h


def rel(a, b):
    return float(np.abs(a - b).max() / np.abs(b).max())


@pytest.mark.gpu
@pytest.mark.parametrize("with_grav", [True, False])
@pytest.mark.parametrize("ref_frame", [0, 1, 2])
@pytest.mark.parametrize("name", list(MODELS))
def test_derivative_tiles(hip_backend, monkeypatch, name, ref_frame, with_grav):
    monkeypatch.setattr(jr, "residual", general_residual)
    table, po, ref, x0, xs, us = _problem(name, 4, 40 + ref_frame, ref_frame, with_grav)
    h = _handle(hip_backend, table, po, ref)
    h.upload_warmstart(xs, us)
    got, want = h.calc_diff(), _reference_tiles(name, table, po, ref, xs, us)
    Lxu, Lqv = _cross_blocks(want, table.nv)
    assert np.abs(Lqv).max() > 1e-6 and (np.abs(Lxu).max() > 1e-6) == with_grav
    _close(got, want, table.nv, name)
    h.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(MODELS))
def test_direction(hip_backend, monkeypatch, name):
    """QP tiles of k_general_rows_wg behind k_calc_qp_wg, k_riccati_blk and k_node_kkt_big_gen against the dense LQR on the
    reference's tiles; the tolerances of tests/test_prismatic_gpu.py::test_direction."""
    monkeypatch.setattr(jr, "residual", general_residual)
    nv = MODELS[name]().nv
    table, po, ref, x0, xs, us = _problem(name, 4 if nv >= 30 else 6, 60 + nv, ref_frame=1)
    h = _handle(hip_backend, table, po, ref)
    h.upload_warmstart(xs, us)
    K, k, dx, du, kkt = h.direction()
    tiles = _reference_tiles(name, table, po, ref, xs, us)
    if name == "gripper":
        Kr, kr, dxr, dur, kktr = jr.direction(nv, tiles)
    else:
        Kr, kr, dxr, dur, kktr = Oracle(table, po, B).direction(tiles)
    print(name, "dx", rel(dx, dxr), "du", rel(du, dur), "K", rel(K, Kr), "kkt", np.abs(kkt / kktr - 1).max())
    assert rel(dx, dxr) < 1e-9 and rel(du, dur) < 1e-9
    assert rel(K, Kr) < 1e-8
    np.testing.assert_allclose(kkt, kktr, rtol=1e-7)
    h.close()


def _same_solve(r_h, r_o):
    for f in ("iter", "solved", "flags"):
        assert np.array_equal(r_h[3][f], r_o[3][f]), (f, r_h[3][f], r_o[3][f])
    print("xs", rel(r_h[0], r_o[0]), "us", np.abs(r_h[1] - r_o[1]).max(), "K", rel(r_h[2], r_o[2]))
    np.testing.assert_allclose(r_h[0], r_o[0], rtol=1e-8, atol=1e-8)
    np.testing.assert_allclose(r_h[1], r_o[1], rtol=1e-8, atol=1e-8)
    assert rel(r_h[2], r_o[2]) <= 1e-7


@pytest.mark.gpu
@pytest.mark.parametrize("seed", [100, 101, 102])
@pytest.mark.parametrize("name", ["tree9", "chain12", "tree16", "humanoid30", "chain31"])
def test_full_solve(hip_backend, name, seed):
    table, po, ref, x0, xs, us = _problem(name, 6, seed)
    h = _handle(hip_backend, table, po, ref)
    r_h = h.solve(x0, xs, us, 30)
    r_o = Oracle(table, po, B).solve(ref, None, x0, xs, us, 30)
    assert np.all(r_o[3]["flags"] == 0) and np.all(r_o[3]["iter"] >= 2) and np.all(r_o[3]["iter"] <= 5)
    _same_solve(r_h, r_o)
    again = h.solve(x0, xs, us, 30)  # no atomics, fixed summation orders: the same bits
    for a, b in zip(r_h[:3], again[:3]):
        assert np.array_equal(a, b)
    assert r_h[3].tobytes() == again[3].tobytes()
    h.close()


def _rejected_step_problem(name, seed):
    table = MODELS[name]()
    nv = table.nv
    po, ref, x0, xs, us = general.general_problem(table, 8, B, seed, 2)
    wi, _, _ = po.row_view(ref, False, 2)  # goal_tracking
    wi *= 1000.0
    x0 = x0.copy()
    x0[:, :nv] += np.random.default_rng(1000 + seed).normal(0, 0.8, (B, nv))
    xs = np.repeat(x0[:, None, :], 9, axis=1)
    return table, po, ref, x0, xs, np.zeros((B, 8, nv))


@pytest.mark.gpu
@pytest.mark.parametrize("name,seed", [("tree9", 26), ("chain12", 6)])
def test_rejected_step_length(hip_backend, name, seed):
    """A stiff goal far from the warm start: the checker rejects step lengths (flags & 4 in one instance), so the trial pass of
    phase 1 -- K1 and k_general_rows_wg at the trial iterate -- runs more than once in an iteration."""
    table, po, ref, x0, xs, us = _rejected_step_problem(name, seed)
    r_o = Oracle(table, po, B).solve(ref, None, x0, xs, us, 30)
    assert np.any(r_o[3]["flags"] & 4), r_o[3]
    h = _handle(hip_backend, table, po, ref)
    _same_solve(h.solve(x0, xs, us, 30), r_o)
    h.close()


@pytest.mark.gpu
def test_filter_line_search(hip_backend):
    table, po0, ref, x0, xs, us = _problem("tree9", 6, 309)
    po = _abi.PackedOcp(9, [0.01] * 6, po0.running, po0.terminal, use_filter_line_search=True)
    h, o = _handle(hip_backend, table, po, ref), Oracle(table, po, B)
    xs_h, us_h, K_h, st_h = h.solve(x0, xs, us, 6)
    xs_o, us_o, K_o, st_o = o.solve(ref, None, x0, xs, us, 6)
    assert np.array_equal(st_h["iter"], st_o["iter"]) and np.array_equal(st_h["flags"], st_o["flags"])
    np.testing.assert_allclose(xs_h, xs_o, rtol=1e-8, atol=1e-10)
    np.testing.assert_allclose(us_h, us_o, rtol=1e-8, atol=1e-8)
    h.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["tree9", "tree16"])
def test_item_costs_and_residuals(hip_backend, name):
    """The two rows' items against the checker that holds the row alone (tests/test_item_costs_gpu.py), their residual vectors
    against the checker's node_calc."""
    import test_item_costs_gpu as items

    table, po0, ref, x0, xs, us = _problem(name, 4, 70, ref_frame=1)
    po = _abi.PackedOcp(table.nv, items.TS, po0.running, po0.terminal)
    h = _handle(hip_backend, table, po, ref)
    h.upload_warmstart(xs, us)
    items._check_items(h, table, po, ref, None, xs, us, TOL16)
    o = Oracle(table, po, B)
    nv = table.nv
    for row in (3, 4):
        res = h.residuals(row)
        off = sum(_abi.row_nr(r.kind, nv) for r in po.running[:row])
        nr = _abi.row_nr(po.running[row].kind, nv)
        for b, t in ((0, 1), (1, 3)):
            _, _, rvec = o.node_calc(False, items.TS[t], xs[b, t], us[b, t], ref[b, t])
            np.testing.assert_allclose(res[b, t], rvec[off:off + nr], atol=1e-10)
    h.close()


@pytest.mark.gpu
def test_resident_sine_trajectory(hip_backend):
    """Three mpc_steps on a resident sine trajectory equal the same steps driven with host tiles and shift_warmstart to 1e-12
    (the form of test_hip_resident_sine_trajectory_with_fourteen_pair_costs)."""
    table, po, ref, x0, xs, us = _problem("tree9", 8, 80)
    T, nv, n_points = 8, 9, 12
    tool = len(table.frame_names) - 1
    q0, amp, puls, scale, t0 = workloads.sine_batch_params(B, nv=nv, q0=np.zeros(nv))
    h = _handle(hip_backend, table, po, ref)
    h.sine_trajectory(n_points, 0.01, q0, amp, puls, scale, t0, np.full(nv, 1.0), np.full(nv, 0.1), np.full(nv, 1e-3), np.full(6, 2.0), tool)
    tiles = np.stack([h.traj_tile(k) for k in range(n_points)], axis=1)
    tiles_t = np.stack([h.traj_tile(k, terminal=True) for k in range(n_points)], axis=1)
    g = _handle(hip_backend, table, po, ref)
    for k in range(3):
        h.mpc_step(k, 10, first=(k == 0))
        r_h = h.download()
        g.set_refs(np.concatenate([tiles[:, k:k + T], tiles_t[:, k + T:k + T + 1]], axis=1))
        if k == 0:
            xs0 = np.stack([np.concatenate(h.traj_point(k + t)[:2], axis=1) for t in range(T + 1)], axis=1)
            us0 = np.stack([h.traj_point(k + t)[3] for t in range(T)], axis=1)
            g.upload_x0(xs0[:, 0])
            g.upload_warmstart(xs0, us0)
        else:
            g.x0_from_prediction()
            g.shift_warmstart()
        g.solve_resident(10)
        r_g = g.download()
        for a, b_ in zip(r_h[:3], r_g[:3]):
            np.testing.assert_allclose(a, b_, rtol=0, atol=1e-12 * max(np.abs(b_).max(), 1.0))
        assert np.array_equal(r_h[3]["iter"], r_g[3]["iter"])
    h.close()
    g.close()


@pytest.mark.gpu
def test_class_surface_from_yaml(hip_backend):
    """OCPCrocoGeneric from a YAML with both items on the nine-joint Panda with unlocked fingers: one solve against the checker."""
    import io

    from agimus_controller_amd.factory.robot_model import RobotModelParameters, RobotModels
    from agimus_controller_amd.ocp.ocp_croco_generic import OCPCrocoGeneric
    from agimus_controller_amd.ocp_param_base import DTFactorsNSeq, OCPParamsBaseCroco
    from agimus_controller_amd.trajectory import TrajectoryPoint, TrajectoryPointWeights, WeightedTrajectoryPoint

    item = "{name: %s, update: true, weight: 1.0, cost: {class: CostModelResidual, residual: {class: %s}, activation: {class: ActivationModelWeightedQuad, weights: 1.0}}}"
    yaml_text = "\n".join([
        "running_model:", "  class: IntegratedActionModelEuler", "  differential:", "    class: DifferentialActionModelFreeFwdDynamics", "    costs:",
        "      - " + item % ("ctrl_grav", "ResidualModelControlGrav"), "      - " + item % ("state_reg", "ResidualModelState"),
        "      - " + item % ("ee_vel", "ResidualModelFrameVelocity, id: panda_hand_tcp, reference_frame: LOCAL_WORLD_ALIGNED"),
        "terminal_model:", "  class: IntegratedActionModelEuler", "  differential:", "    class: DifferentialActionModelFreeFwdDynamics", "    costs:",
        "      - " + item % ("state_reg", "ResidualModelState")]) + "\n"
    table = sizes._model(9, "panda_fingers")
    rm = RobotModels(RobotModelParameters(table=table, q0=np.zeros(9), armature=table.armature))
    T = 8
    params = OCPParamsBaseCroco(dt=0.01, horizon_size=T, dt_factor_n_seq=DTFactorsNSeq(factors=[1], n_steps=[T]), solver_iters=30, callbacks=False)
    ocp = OCPCrocoGeneric(rm, params, io.StringIO(yaml_text))
    assert [r.kind for r in ocp.problem.running] == [_abi.RES_CONTROL_GRAV, _abi.RES_STATE, _abi.RES_FRAME_VELOCITY]
    q = np.concatenate([workloads.PANDA_Q0, [0.1, -0.1]])
    pt = WeightedTrajectoryPoint(
        TrajectoryPoint(robot_configuration=q, robot_velocity=np.zeros(9), robot_effort=np.zeros(9),
                        end_effector_velocities={"panda_hand_tcp": np.array([0.05, -0.02, 0.03, 0.0, 0.0, 0.1])}),
        TrajectoryPointWeights(w_robot_configuration=np.ones(9), w_robot_velocity=0.1 * np.ones(9), w_robot_effort=1e-3 * np.ones(9),
                               w_end_effector_velocities={"panda_hand_tcp": 5.0 * np.ones(6)}))
    ocp.set_reference_weighted_trajectory([pt] * (T + 1))
    x0 = np.concatenate([q, np.zeros(9)])
    ocp.solve(x0, [x0] * (T + 1), [np.zeros(9)] * T)
    assert ocp._hip.general_rows
    o = Oracle(table, ocp.problem, 1)
    xs_o, us_o, K_o, st_o = o.solve(ocp._ref_tile, ocp._frames, x0[None], np.tile(x0, (1, T + 1, 1)), np.zeros((1, T, 9)), 30)
    assert ocp.debug_data.nb_iter == st_o["iter"][0]
    np.testing.assert_allclose(np.array(ocp.ocp_results.states), xs_o[0], rtol=1e-7, atol=1e-9)
    np.testing.assert_allclose(np.array(ocp.ocp_results.feed_forward_terms), us_o[0], rtol=1e-6, atol=1e-8)


@pytest.mark.gpu
def test_refusals(hip_backend):
    table, po, ref, x0, xs, us = _problem("tree9", 4, 90)
    lim = np.full(9, 20.0)
    con = [_abi.ConstraintSpec(_abi.RES_CONTROL, lower=-lim, upper=lim, name="ctrl_limit")]
    with pytest.raises(Exception, match=r"(FrameVelocity|ControlGrav) cost row.*7 joints"):
        hip_backend.HipOcp(table, _abi.PackedOcp(9, [0.01] * 4, po.running, po.terminal, running_constraints=con), B)
    import dataclasses

    exp = [dataclasses.replace(r, activation=_abi.ACT_EXP, alpha=2.0) if r.kind == _abi.RES_CONTROL_GRAV else r for r in po.running]
    with pytest.raises(Exception, match="ControlGrav"):
        hip_backend.HipOcp(table, _abi.PackedOcp(9, [0.01] * 4, exp, po.terminal), B)
    t32 = MODELS["chain32"]()
    po5 = general.general_problem(t32, 4, B, 1)[0]
    assert po5.stride > 256
    with pytest.raises(Exception, match="256"):
        hip_backend.HipOcp(t32, po5, B)


_NO_CHANGE_CHILD = """
import sys
import numpy as np
sys.path[:0] = [sys.argv[2], sys.argv[2] + "/tests"]
from agimus_controller_amd import backend, workloads
import test_general_rows_large as t
out = {}
for name in ("tree9", "humanoid30"):
    table = t.MODELS[name]()
    po, ref, x0, xs, us = workloads.random_goal_problem(table, 6, 0.01, t.B, seed=5, frame=len(table.frame_names) - 1)
    h = backend.HipOcp(table, po, t.B)
    h.set_refs(ref)
    h.upload_warmstart(xs, us)
    out[name + "_tiles"] = h.calc_diff()
    r = h.solve(x0, xs, us, 10)
    out[name + "_xs"], out[name + "_us"], out[name + "_K"], out[name + "_status"] = r[0], r[1], r[2], np.frombuffer(r[3].tobytes(), dtype=np.uint8)
    h.close()
np.savez(sys.argv[1], **out)
"""


@pytest.mark.gpu
def test_a_handle_without_general_rows_takes_the_path_it_took(hip_backend, tmp_path):
    """No general row (nv = 9 at the 16-joint capacity, and the 30-joint humanoid): agx_ocp_general_rows == 0, and calc_diff tiles,
    xs, us, K and the status words of a solve are bitwise those of the library built with the launch sites of the new kernels
    compiled out (backend.NOGEN_LIB_PATH: -DAGX_NO_GENERAL_ROWS, there K1 also reads d_ocp as it did).  Each library in a fresh
    child process, through AGX_LIB.  That variant refuses a handle with general rows above 7 joints."""
    import os
    import pathlib
    import subprocess
    import sys

    table = MODELS["tree9"]()
    po, ref, x0, xs, us = workloads.random_goal_problem(table, 6, 0.01, B, seed=5, frame=len(table.frame_names) - 1)
    h = hip_backend.HipOcp(table, po, B)
    assert not h.general_rows and hip_backend.lib().agx_ocp_general_rows(h._h) == 0
    h.set_refs(ref)
    h.upload_warmstart(xs, us)
    Lxu, Lqv = _cross_blocks(h.calc_diff(), 9)
    assert not Lxu.any() and not Lqv.any()
    h.close()
    root = pathlib.Path(__file__).resolve().parent.parent
    assert hip_backend.NOGEN_LIB_PATH.exists(), "backend.build() makes the library with the launch sites compiled out"
    res = {}
    for tag, lib in (("with", hip_backend.LIB_PATH), ("without", hip_backend.NOGEN_LIB_PATH)):
        env = dict(os.environ, AGX_LIB=str(lib))
        out = tmp_path / f"{tag}.npz"
        subprocess.run([sys.executable, "-c", _NO_CHANGE_CHILD, str(out), str(root)], env=env, check=True, timeout=120)
        res[tag] = np.load(out)
    assert sorted(res["with"].files) == sorted(res["without"].files) and len(res["with"].files) == 10
    for k in res["with"].files:
        assert np.array_equal(res["with"][k], res["without"][k]), k
    # the variant has no quiet fall-back for the rows it leaves out
    child = ("import sys; sys.path[:0] = [sys.argv[1], sys.argv[1] + '/tests']\n"
             "from agimus_controller_amd import backend\nimport test_general_rows_large as t\n"
             "table, po, ref, x0, xs, us = t._problem('tree9', 4, 90)\n"
             "try:\n    backend.HipOcp(table, po, t.B)\nexcept backend.HipError as e:\n    sys.exit(0 if 'compiled out' in str(e) else 2)\nsys.exit(1)\n")
    rc = subprocess.run([sys.executable, "-c", child, str(root)], env=dict(os.environ, AGX_LIB=str(hip_backend.NOGEN_LIB_PATH)), timeout=120).returncode
    assert rc == 0, rc
