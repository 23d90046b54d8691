"""Collision avoidance with many collision-pair constraints per node (wide constraint sets, DESIGN.md section on constraints).

Up to 64 collision-distance rows next to one State and one Control row run on the 7-joint capacity with their own layout
(k_con_eval_pairs and the WIDE instances of the ADMM node kernels).  As every constrained path, parity with the reference
binaries is UNPINNED: the HIP path is checked against the project's CPU checker under oracle/.
"""
import ctypes as C
import dataclasses

import numpy as np
import pytest

from agimus_controller_amd import _abi, workloads
from agimus_controller_amd.factory import robot_tables as rt

CAPSULES = workloads.PANDA_LINK_CAPSULES
SELF_PAIRS = workloads.PANDA_SELF_COLLISION_PAIRS


def _table(n_obstacles):
    return rt.panda_collision_table(0.1, obstacle_xyz=(0.45, 0.1, 0.45), obstacle_radius=0.08, obstacle_length=0.3,
                                    obstacles=workloads.random_obstacles(n_obstacles))


def _pairs12():
    return [(c, "obstacle") for c in CAPSULES] + [(c, "ob0") for c in CAPSULES] + SELF_PAIRS[:2]


LOWER12 = 0.0475  # two link capsules of the first instance start 0.048 from obstacle ob0


def _pairs64():
    return [(c, f"ob{i}") for i in range(12) for c in CAPSULES] + SELF_PAIRS


def _problem(table, pairs, lower=0.02, T=10, B=3, seed=23, with_state=True, with_control=True, max_qp=100):
    tcp = table.frame_id("panda_hand_tcp")
    running, terminal = workloads.collision_avoidance_rows(table, tcp, alpha=0.05)
    con = []
    if with_state:
        con.append(_abi.ConstraintSpec(_abi.RES_STATE, lower=-5.0, upper=5.0, name="box"))
    if with_control:
        lim = np.asarray(table.effort_limit, dtype=float)
        con.append(_abi.ConstraintSpec(_abi.RES_CONTROL, lower=-lim, upper=lim, name="torque"))
    con += workloads.collision_pair_constraints(table, pairs, lower)
    po = _abi.PackedOcp(7, [0.01] * T, running, terminal, max_qp_iters=max_qp, running_constraints=con, terminal_constraints=con)
    _, ref, x0, xs, us = workloads.random_goal_problem(table, T, 0.01, B, seed, frame=tcp, rows="collision")
    return po, ref, x0, xs, us


def _oracle(table, po, B):
    from oracle.oracle import Oracle

    return Oracle(table, po, B)


def _distances(o, n_pairs, terminal, x, u=None):
    """The last n_pairs constraint components of a node (collision distances) from the checker, with buffers sized for any
    number of rows."""
    from oracle.oracle import _p, lib

    x = np.ascontiguousarray(x, dtype=float)
    u = np.zeros(o.nu) if u is None else np.ascontiguousarray(u, dtype=float)
    n = 3 * o.nv + n_pairs + 8
    g, Gx, Gu, nc = np.zeros(n), np.zeros((n, o.nx)), np.zeros((n, o.nu)), C.c_int(0)
    lib().orc_node_constraints(o._h, int(terminal), _p(x), _p(u), _p(g), _p(Gx), _p(Gu), C.byref(nc))
    assert nc.value <= n
    return g[nc.value - n_pairs:nc.value]


def _assert_matches_checker(r_h, r_o):
    """The tolerances of test_constraints.py::test_hip_collision_constraint_matches_the_checker."""
    assert np.array_equal(r_h[3]["qp_iters"], r_o[3]["qp_iters"])
    np.testing.assert_allclose(r_h[0], r_o[0], rtol=1e-7, atol=1e-8)
    np.testing.assert_allclose(r_h[1], r_o[1], rtol=1e-6, atol=1e-6)
    np.testing.assert_allclose(r_h[2], r_o[2], rtol=1e-5, atol=1e-5)
    np.testing.assert_allclose(r_h[3]["kkt"], r_o[3]["kkt"], rtol=1e-5, atol=1e-8)


# ------------------------------------------------------------------------------------------------------------- CPU
def test_yaml_lowers_twelve_collision_items():
    from agimus_controller_amd.factory.robot_model import RobotModelParameters, RobotModels
    from agimus_controller_amd.ocp import ocp_croco_generic as g

    table = _table(2)
    pairs = _pairs12()
    rm = RobotModels(RobotModelParameters(table=table, armature=table.armature, collision_pairs=pairs))
    items = [{"name": f"collision_{i}", "constraint": {"class": "ConstraintModelResidual", "lower": 0.02, "upper": "inf",
                                                         "residual": {"class": "ResidualDistanceCollision", "collision_pair_id": i}}}
             for i in range(len(pairs))]
    diff = g.create_croco_dataclasses({
        "class": "DifferentialActionModelFreeFwdDynamics",
        "costs": [{"name": "state_reg", "cost": {"class": "CostModelResidual", "residual": {"class": "ResidualModelState"}}}],
        "constraints": items,
    })
    data = g.BuildData(rm.robot_model, 7, rm.collision_model)
    run, term = diff.lower_constraints(data, False), diff.lower_constraints(data, True)
    assert len(run) == 12 and all(c.kind == _abi.RES_COLLISION for c in run)
    assert [(c.frame, c.frame_b) for c in run] == [(table.frame_id(a), table.frame_id(b)) for a, b in pairs]
    assert all(c.active for c in term)
    po = _abi.PackedOcp(7, [0.01] * 4, diff.lower(data), diff.lower(data), running_constraints=run, terminal_constraints=term)
    assert po.desc.n_running_constraints == 12 and po.desc.n_terminal_constraints == 12
    # the same rows through the Python helper
    helper = workloads.collision_pair_constraints(table, pairs, 0.02)
    assert [(c.frame, c.frame_b, c.lower, c.upper) for c in helper] == [(c.frame, c.frame_b, 0.02, np.inf) for c in run]


def test_checker_keeps_twelve_pairs_apart():
    table = _table(2)
    pairs = _pairs12()
    po, ref, x0, xs, us = _problem(table, pairs, lower=LOWER12)
    o = _oracle(table, po, 3)
    xs_c, us_c, K, st = o.solve(ref, None, x0, xs, us, 30)
    assert np.all(st["solved"] == 1)
    assert np.all(st["kkt"] <= 1e-3)
    T = po.horizon
    d = np.array([[_distances(o, len(pairs), t == T, xs_c[b, t], None if t == T else us_c[b, t]) for t in range(1, T + 1)]
                  for b in range(3)])
    assert d.min() >= LOWER12 - 1e-6
    # the bound shapes the solve: with a loose one the first instance ends elsewhere
    po_l, *_ = _problem(table, pairs, lower=0.02)
    xs_l = _oracle(table, po_l, 3).solve(ref, None, x0, xs, us, 30)[0]
    assert np.abs(xs_l[0] - xs_c[0]).max() > 1e-4


def test_obstacles_keyword_keeps_the_default_table():
    a, b = rt.panda_collision_table(0.1), rt.panda_collision_table(0.1, obstacles=())
    assert a.frame_names == b.frame_names
    np.testing.assert_array_equal(a.frame_placement, b.frame_placement)
    t = _table(12)
    assert len(t.frame_names) == len(a.frame_names) + 12
    assert t.frame_box[t.frame_id("ob2")][0] > 0 and t.frame_radius[t.frame_id("ob1")] > 0


# ------------------------------------------------------------------------------------------------------------- GPU
@pytest.mark.gpu
@pytest.mark.parametrize("admm_loop", [None, "2"])
def test_hip_twelve_pairs_state_box_and_torque_limits_match_the_checker(monkeypatch, admm_loop):
    """admm_loop "2": the gradient-only ADMM iterations of every instance in k_admm_loop (its WIDE instance), as
    test_constraints.py::test_hip_admm_iterations_in_one_launch_are_the_same_solve does for the fixed layout."""
    from agimus_controller_amd import backend

    if admm_loop is not None:
        monkeypatch.setenv("AGX_ADMM_LOOP", admm_loop)
    table = _table(2)
    po, ref, x0, xs, us = _problem(table, _pairs12(), lower=LOWER12)
    o = _oracle(table, po, 3)
    hb = backend.HipOcp(table, po, 3)
    hb.set_refs(ref)
    r_o = o.solve(ref, None, x0, xs, us, 2)
    r_h = hb.solve(x0, xs, us, 2)
    _assert_matches_checker(r_h, r_o)
    if admm_loop is not None:
        assert r_h[3]["qp_iters"].max() > 25  # gradient-only iterations past the first rho check: k_admm_loop ran
    hb.close()


@pytest.mark.gpu
def test_hip_sixty_four_pairs_match_the_checker_also_on_a_moved_obstacle_scene():
    from agimus_controller_amd import backend

    table = _table(12)
    pairs = _pairs64()
    assert len(pairs) == 64
    po, ref, x0, xs, us = _problem(table, pairs)
    o = _oracle(table, po, 3)
    hb = backend.HipOcp(table, po, 3)
    hb.set_refs(ref)
    r_o = o.solve(ref, None, x0, xs, us, 2)
    r_h = hb.solve(x0, xs, us, 2)
    _assert_matches_checker(r_h, r_o)
    # move one obstacle: on the checker only the distances of its pairs change; after set_geom_placement the device solves as
    # the checker does on the moved scene (the device's constraint values are not read back one by one)
    f = table.frame_id("ob4")
    moved = np.asarray(table.frame_placement, dtype=float).reshape(-1, 12).copy()
    moved[f, 9:] += np.array([-0.05, 0.04, 0.03])
    table2 = dataclasses.replace(table, frame_placement=moved)
    o2 = _oracle(table2, po, 3)
    d1 = _distances(o, len(pairs), False, x0[0], us[0, 0])
    d2 = _distances(o2, len(pairs), False, x0[0], us[0, 0])
    mine = np.array([b == "ob4" for _, b in pairs])
    assert np.all(d1[~mine] == d2[~mine]) and np.all(d1[mine] != d2[mine])
    hb.set_geom_placement(f, moved[f])
    hb.reset_duals()
    r_o2 = o2.solve(ref, None, x0, xs, us, 2)
    r_h2 = hb.solve(x0, xs, us, 2)
    _assert_matches_checker(r_h2, r_o2)
    assert not np.allclose(r_h2[0], r_h[0], rtol=0, atol=1e-12)
    hb.close()


@pytest.mark.gpu
@pytest.mark.parametrize("row", ["state", "control"])
def test_hip_wide_layout_forced_on_a_small_set_is_the_same_solve(monkeypatch, row):
    """A set that fits the fixed layout (three pairs and a State or a Control row: four rows) solved there and, with
    AGX_CON_WIDE=1, on the wide layout: identical iteration counts, results equal up to round-off."""
    from agimus_controller_amd import backend

    table = _table(2)
    pairs = [("panda_link7_capsule_0", "obstacle"), ("panda_link5_capsule_0", "obstacle"), ("panda_link7_capsule_0", "ob0")]
    po, ref, x0, xs, us = _problem(table, pairs, lower=LOWER12, with_state=row == "state", with_control=row == "control")
    out = {}
    for wide in ("0", "1"):
        monkeypatch.setenv("AGX_CON_WIDE", wide)
        hb = backend.HipOcp(table, po, 3)
        hb.set_refs(ref)
        out[wide] = hb.solve(x0, xs, us, 6)
        hb.close()
    a, b = out["0"], out["1"]
    for key in ("iter", "qp_iters", "solved", "flags"):
        assert np.array_equal(a[3][key], b[3][key]), key
    for i in range(3):
        np.testing.assert_allclose(b[i], a[i], rtol=0, atol=1e-12)
    np.testing.assert_allclose(b[3]["kkt"], a[3]["kkt"], rtol=1e-12, atol=1e-12)


@pytest.mark.gpu
def test_hip_terminal_control_grav_row_next_to_pairs_is_left_out_as_on_the_fixed_layout():
    """The terminal node has no control: a ControlGrav constraint there is left out (as crocoddyl does with nu = 0) whatever the
    layout, so a terminal set of ten pairs plus a ControlGrav row solves exactly as the ten pairs alone.  On a running node the
    row is a kind the wide layout does not take: refused."""
    from agimus_controller_amd import backend

    table = _table(2)
    pairs = _pairs12()[:10]
    tcp = table.frame_id("panda_hand_tcp")
    running, terminal = workloads.collision_avoidance_rows(table, tcp, alpha=0.05)
    con = workloads.collision_pair_constraints(table, pairs, LOWER12)
    grav = _abi.ConstraintSpec(_abi.RES_CONTROL_GRAV, lower=-4.0, upper=4.0, name="tau_minus_g")
    _, ref, x0, xs, us = workloads.random_goal_problem(table, 10, 0.01, 3, 23, frame=tcp, rows="collision")
    out = []
    for term in (con, con + [grav], con + [grav, grav]):
        po = _abi.PackedOcp(7, [0.01] * 10, running, terminal, max_qp_iters=100, running_constraints=con, terminal_constraints=term)
        hb = backend.HipOcp(table, po, 3)
        hb.set_refs(ref)
        out.append(hb.solve(x0, xs, us, 2))
        hb.close()
    for r in out[1:]:
        for key in ("iter", "qp_iters", "solved", "flags"):
            assert np.array_equal(r[3][key], out[0][3][key]), key
        for i in range(3):
            np.testing.assert_array_equal(r[i], out[0][i])
    po = _abi.PackedOcp(7, [0.01] * 10, running, terminal, running_constraints=con + [grav], terminal_constraints=con)
    with pytest.raises(backend.HipError, match="at most 4 active constraint rows"):
        backend.HipOcp(table, po, 1)


def _with_capsules(table, n):
    """table plus n link capsules (on joints 1, 2, ...) and n sphere obstacles."""
    for i in range(n):
        table = table.with_geometry(f"cap{i}", 1 + i % (table.nv - 1), rt.se3(None, [0.0, 0.0, 0.05]), 0.04, 0.05)
    for i in range(n):
        table = table.with_geometry(f"sph{i}", -1, rt.se3(None, [0.4, 0.1 * i, 0.3]), 0.05)
    return table


@pytest.mark.gpu
def test_hip_refuses_what_the_wide_layout_does_not_cover():
    from agimus_controller_amd import backend

    # a 65th pair
    table = _table(13)
    pairs = [(c, f"ob{i}") for i in range(13) for c in CAPSULES]
    assert len(pairs) == 65
    po, *_ = _problem(table, pairs, T=4, B=1)
    with pytest.raises(backend.HipError, match="at most 64 collision-pair"):
        backend.HipOcp(table, po, 1)
    # a frame-translation row next to ten pairs
    table = _table(2)
    tcp = table.frame_id("panda_hand_tcp")
    running, terminal = workloads.goal_reaching_rows(tcp)
    con = workloads.collision_pair_constraints(table, _pairs12()[:10], 0.02)
    con.append(_abi.ConstraintSpec(_abi.RES_FRAME_TRANSLATION, lower=-0.1, upper=0.1, ref=[0.4, 0.0, 0.4], frame=tcp, name="ee_box"))
    with pytest.raises(backend.HipError, match="at most 4 active constraint rows"):
        backend.HipOcp(table, _abi.PackedOcp(7, [0.01] * 4, running, terminal, running_constraints=con), 1)
    # ten pairs on a tree model and on a 9-joint chain
    for base in (rt.tree_table(7, seed=3), rt.chain_table(9, seed=4)):
        t = _with_capsules(base, 5)
        pairs = [(f"cap{i}", f"sph{j}") for i in range(5) for j in range(2)]
        con = workloads.collision_pair_constraints(t, pairs, 0.01)
        run, term = workloads.regulation_rows()
        with pytest.raises(backend.HipError, match="at most 4 active constraint rows"):
            backend.HipOcp(t, _abi.PackedOcp(t.nv, [0.01] * 4, run, term, running_constraints=con), 1)


@pytest.mark.gpu
def test_hip_resident_mpc_loop_with_twenty_pairs_stays_feasible():
    from agimus_controller_amd import backend

    # the sphere obstacle of bench.py --workload collision, where the link-7 capsule of part of the batch comes close
    table = rt.panda_collision_table(0.1, obstacle_xyz=(0.27, 0.22, 0.70), obstacle_radius=0.06, obstacle_length=0.0,
                                     obstacles=workloads.random_obstacles(3))
    pairs = [(c, "obstacle") for c in CAPSULES] + [(c, f"ob{i}") for i in range(3) for c in CAPSULES]
    assert len(pairs) == 20
    lower = 0.01
    T, B = 40, 8
    tcp = table.frame_id("panda_hand_tcp")
    running, terminal = workloads.collision_avoidance_rows(table, tcp, alpha=1e-4)
    con = workloads.collision_pair_constraints(table, pairs, lower)
    po = _abi.PackedOcp(7, [0.01] * T, running, terminal, termination_tolerance=1e-3, max_qp_iters=100, running_constraints=con,
                        terminal_constraints=con)
    hb = backend.HipOcp(table, po, B)
    q0, amp, puls, scale, t0 = workloads.sine_batch_params(B, lower=table.lower_position_limit, upper=table.upper_position_limit)
    w = workloads.SINE_WEIGHTS
    hb.sine_trajectory(T + 30, 0.01, q0, amp, puls, scale, t0, w["w_q"], w["w_qdot"], w["w_effort"], w["w_pose"], tcp)
    o = _oracle(table, po, 1)
    worst = np.inf
    for k in range(20):
        hb.mpc_step(k, 10, first=(k == 0))
        xs = hb.download(want_K=False)[0]
        assert np.all(np.isfinite(xs))
        for b in range(B):
            for t in range(1, T + 1):
                worst = min(worst, _distances(o, len(pairs), t == T, xs[b, t]).min())
    assert worst >= lower - 1e-4, worst
    hb.close()
