"""Soft collision avoidance with many collision-pair COSTS per node (wide cost sets).

Up to 64 ResidualDistanceCollision cost rows (QuadExp / Exp activation) behind up to 8 other rows run on the 7-joint capacity:
K1 on the prefix of the row table, k_cost_pairs adds the pairs into the tiles.  The CPU checker's analytic leg copies the rows of
7- and 30-joint models into a table of 8, so every comparison with more than 8 rows uses a 6-joint chain (padded to the 7-joint
capacity: the same kernels); the Panda cases stay at 8 rows and compare AGX_COST_WIDE=1 with the default path.
"""
import ctypes as C

import numpy as np
import pytest

from agimus_controller_amd import _abi, workloads
from agimus_controller_amd.factory import robot_tables as rt

B = 3
CAPS = [f"cap{j}" for j in range(1, 6)]
SELF = [("cap1", "cap3"), ("cap1", "cap4"), ("cap1", "cap5"), ("cap2", "cap5")]
SOLVE_SEED = 71  # chosen on the CPU: the checker rejects a step length (status bit 2) in the 64-pair solve; seeds 0 .. 119 give none with 24


def _chain():
    """chain_table(6, seed=3) with a capsule (r 0.04, half length 0.06) on joints 1 .. 5 and twelve seeded world capsules,
    spheres and boxes."""
    t = rt.chain_table(6, seed=3)
    for j in range(1, 6):
        t = t.with_geometry(f"cap{j}", j, rt.se3(None, [0.0, 0.0, 0.05]), 0.04, 0.06)
    rng = np.random.default_rng(5)
    for i in range(12):
        d = rng.normal(size=3)
        xyz = list(rng.uniform(0.45, 0.9) * d / np.linalg.norm(d))
        if i % 3 == 0:
            t = t.with_geometry(f"ob{i}", -1, rt.se3(rt.rpy(0.0, np.pi / 2, 0.0), xyz), rng.uniform(0.03, 0.07), rng.uniform(0.05, 0.15))
        elif i % 3 == 1:
            t = t.with_geometry(f"ob{i}", -1, rt.se3(None, xyz), rng.uniform(0.03, 0.07), 0.0)
        else:
            t = t.with_geometry(f"ob{i}", -1, rt.se3(None, xyz), box=tuple(rng.uniform(0.03, 0.08, 3)))
    return t


def _pairs(n):
    """n pairs: the four self pairs first, then link capsule x obstacle."""
    world = [(c, f"ob{i}") for i in range(12) for c in CAPS]
    out = (SELF + world)[:n]
    assert len(out) == n
    return out


def _rows(table, n, activation=_abi.ACT_QUAD_EXP, alpha=0.05, inactive=None):
    tool = table.frame_id("tool")
    running, terminal = workloads.goal_reaching_rows(tool)
    pc = workloads.collision_pair_costs(table, _pairs(n), activation, alpha, 0.1)
    if inactive is not None:
        pc[inactive].active = False
    return list(running) + pc, list(terminal) + pc


def _problem(table, n, T=10, seed=SOLVE_SEED, **kw):
    run, term = _rows(table, n, **kw)
    return workloads.random_goal_problem(table, T, 0.01, B, seed, frame=table.frame_id("tool"), rows=(run, term))


def _oracle(table, po, batch=B):
    from oracle.oracle import Oracle

    return Oracle(table, po, batch)


_CHECKER = {}


def _checker_solve(n):
    """The checker's 30-iteration solve of the n-pair problem (computed once, shared, left unchanged)."""
    if n not in _CHECKER:
        table = _chain()
        po, ref, x0, xs, us = _problem(table, n)
        _CHECKER[n] = (table, po, ref, x0, xs, us, _oracle(table, po).solve(ref, None, x0, xs, us, 30))
    return _CHECKER[n]


# ------------------------------------------------------------------------------------------------------------- CPU
def test_packed_ocp_takes_three_plus_sixty_four_rows():
    table = _chain()
    run, term = _rows(table, 64)
    assert len(run) == 3 + 64
    po = _abi.PackedOcp(6, [0.01] * 4, run, term)
    prefix = sum(r.width(6) for r in run[:3])
    assert po.stride == prefix + 128
    assert po.desc.n_running_rows == 67
    ref = po.new_ref_tile(2)
    for p in (0, 1, 63):
        wi, rr, aw = po.row_view(ref, False, 3 + p)
        assert po.running_offsets[3 + p] == prefix + 2 * p
        assert rr.shape[-1] == 0 and aw.shape[-1] == 1
        assert np.all(wi == 0.1) and np.all(aw == 1.0)
        wi[...] = 7.0 + p
        assert np.all(ref[:, :4, prefix + 2 * p] == 7.0 + p)
    tprefix = sum(r.width(6) for r in term[: len(term) - 64])
    assert po.terminal_offsets[-1] == tprefix + 126


def test_packed_ocp_refuses_what_a_wide_cost_set_does_not_cover():
    table = _chain()
    run, term = _rows(table, 64)
    extra = workloads.collision_pair_costs(table, [("cap5", "ob11")])
    with pytest.raises(ValueError, match="at most 64 collision-pair"):
        _abi.PackedOcp(6, [0.01] * 4, run + extra, term)
    other = [_abi.RowSpec(_abi.RES_STATE, name=f"s{i}") for i in range(9)]
    with pytest.raises(ValueError, match="at most 8 cost items that are not collision"):
        _abi.PackedOcp(6, [0.01] * 4, other + run[3:], term)
    with pytest.raises(ValueError, match="must come last.*collision_cost_0"):
        _abi.PackedOcp(6, [0.01] * 4, run[3:12] + run[:3], term)
    _abi.PackedOcp(6, [0.01] * 4, run[3:8] + run[:3], term[:2])  # eight rows in any order: the row table, as before
    # one node type over the row table makes the set wide as a whole: the short table follows the wide rule too, as at create
    with pytest.raises(ValueError, match="terminal rows.*must come last"):
        _abi.PackedOcp(6, [0.01] * 4, run, run[3:5] + term[:2])
    _abi.PackedOcp(6, [0.01] * 4, run, term[:2] + run[3:5])


def _yaml_diff(n_pairs, order="last"):
    from agimus_controller_amd.ocp import ocp_croco_generic as g

    coll = [{"name": f"collision_{i}", "weight": 0.1,
             "cost": {"class": "CostModelResidual", "activation": {"class": "ActivationModelQuadExp", "alpha": 0.05},
                      "residual": {"class": "ResidualDistanceCollision", "collision_pair_id": i}}} for i in range(n_pairs)]
    state = [{"name": "state_reg", "cost": {"class": "CostModelResidual", "residual": {"class": "ResidualModelState"}}}]
    return g.create_croco_dataclasses({"class": "DifferentialActionModelFreeFwdDynamics",
                                       "costs": state + coll if order == "last" else coll + state})


def test_yaml_lowers_twelve_collision_cost_items():
    from agimus_controller_amd.factory.robot_model import RobotModelParameters, RobotModels
    from agimus_controller_amd.ocp import ocp_croco_generic as g

    table = _chain()
    pairs = _pairs(12)
    rm = RobotModels(RobotModelParameters(table=table, armature=table.armature, collision_pairs=pairs))
    data = g.BuildData(rm.robot_model, 6, rm.collision_model)
    rows = _yaml_diff(12).lower(data)
    assert len(rows) == 13 and all(r.kind == _abi.RES_COLLISION for r in rows[1:])
    assert [(r.frame, r.frame_b) for r in rows[1:]] == [(table.frame_id(a), table.frame_id(b)) for a, b in pairs]
    assert all(r.activation == _abi.ACT_QUAD_EXP and r.alpha == 0.05 and r.weight == 0.1 for r in rows[1:])
    helper = workloads.collision_pair_costs(table, pairs, _abi.ACT_QUAD_EXP, 0.05, 0.1)
    assert [(r.frame, r.frame_b, r.alpha, r.weight) for r in helper] == [(r.frame, r.frame_b, r.alpha, r.weight) for r in rows[1:]]
    with pytest.raises(ValueError, match="must come last.*collision_0"):
        _yaml_diff(12, order="first").lower(data)
    rm65 = RobotModels(RobotModelParameters(table=table, armature=table.armature, collision_pairs=_pairs(64) + [("cap3", "cap5")]))
    with pytest.raises(ValueError, match="at most 64 collision-pair"):
        _yaml_diff(65).lower(g.BuildData(rm65.robot_model, 6, rm65.collision_model))


def test_checker_converges_with_twenty_four_pair_costs_and_they_shape_the_solve():
    table, po, ref, x0, xs, us, (xs_c, us_c, K_c, st) = _checker_solve(24)
    assert np.all(st["solved"] == 1) and np.all(st["kkt"] <= 1e-3)
    # a rejected step length (status bit 2) in an instance of the 64-pair solve: its GPU run goes through a second trial pass
    st64 = _checker_solve(64)[6][3]
    assert np.all(st64["solved"] == 1) and np.any(st64["flags"] & 4), st64["flags"]
    ref0 = ref.copy()
    for term in (False, True):
        for p in range(24):
            po.row_view(ref0, term, len(po.terminal if term else po.running) - 24 + p)[0][...] = 0.0
    xs_0 = _oracle(table, po).solve(ref0, None, x0, xs, us, 30)[0]
    assert np.abs(xs_0 - xs_c).max() > 1e-3


# ------------------------------------------------------------------------------------------------------------- GPU
def _assert_tiles(got, want, nv):
    for field, s in _abi.tile_slices(nv).items():
        scale = max(np.abs(want[..., s]).max(), 1e-300)
        err = np.abs(got[..., s] - want[..., s]).max()
        print(field, err / scale)
        assert err <= 1e-10 * scale + 1e-13, field


@pytest.mark.gpu
@pytest.mark.parametrize("activation,alpha", [(_abi.ACT_QUAD_EXP, 0.05), (_abi.ACT_EXP, 0.1)])
@pytest.mark.parametrize("n", [9, 14, 64])
def test_hip_canonical_tiles_with_pair_costs_match_the_checker(hip_backend, n, activation, alpha):
    """agx_ocp_calc_diff, terminal node included, one inactive row in the middle of the set; 1e-10 (padded sizes)."""
    table = _chain()
    po, ref, x0, xs, us = _problem(table, n, T=4, activation=activation, alpha=alpha, inactive=n // 2)
    h, o = hip_backend.HipOcp(table, po, B), _oracle(table, po)
    h.set_refs(ref)
    h.upload_warmstart(xs, us)
    got, want = h.calc_diff(), o.calc_diff(ref, None, xs, us)
    _assert_tiles(got, want, 6)
    # the pair rows are in it: without them the Lx block differs
    ref0 = ref.copy()
    for p in range(n):
        po.row_view(ref0, False, 3 + p)[0][...] = 0.0
    sl = _abi.tile_slices(6)["Lxx"]
    assert np.abs(o.calc_diff(ref0, None, xs, us)[..., sl] - want[..., sl]).max() > 1e-6
    # the distance of a pair row through agx_ocp_get_residuals: the checker's constraint value of the same pair
    d = h.residuals(3 + 1)
    assert d.shape == (B, 4, 1)
    con = workloads.collision_pair_constraints(table, _pairs(n)[1:2], 0.0)
    oc = _oracle(table, _abi.PackedOcp(6, [0.01] * 4, po.running[:3], po.terminal[:2], running_constraints=con), 1)
    from oracle.oracle import _p, lib

    g, Gx, Gu, nc = np.zeros(8), np.zeros((8, 12)), np.zeros((8, 6)), C.c_int(0)
    for b in range(B):
        for t in range(4):
            lib().orc_node_constraints(oc._h, 0, _p(np.ascontiguousarray(xs[b, t])), _p(np.ascontiguousarray(us[b, t])), _p(g), _p(Gx), _p(Gu),
                                       C.byref(nc))
            assert abs(d[b, t, 0] - g[nc.value - 1]) <= 1e-12
    h.close()


def _panda_problem(T=10):
    table = rt.panda_collision_table(0.1, obstacle_xyz=(0.45, 0.1, 0.45), obstacle_radius=0.08, obstacle_length=0.3,
                                     obstacles=workloads.random_obstacles(2))
    tcp = table.frame_id("panda_hand_tcp")
    running, terminal = workloads.goal_reaching_rows(tcp)
    pairs = [(c, "obstacle") for c in workloads.PANDA_LINK_CAPSULES[2:]] + [("panda_link7_capsule_0", "ob0"), ("panda_link5_capsule_0", "ob1")]
    pc = workloads.collision_pair_costs(table, pairs, _abi.ACT_QUAD_EXP, 0.05, 0.1)
    assert len(running) + len(pc) == 8
    return (table,) + tuple(workloads.random_goal_problem(table, T, 0.01, B, 23, frame=tcp, rows=(list(running) + pc, list(terminal) + pc)))


@pytest.mark.gpu
def test_hip_panda_three_plus_five_rows_wide_path_is_the_default_solve(hip_backend, monkeypatch):
    """qp_tiles and a full solve with AGX_COST_WIDE=1 against the default path (rtol 1e-12) and against the checker.
    The two paths sum the pairs in a different order, so an entry that is a sum of terms cancelling to something small carries
    an error of 1e-16 times the TERMS, not times the entry: next to rtol 1e-12 the comparison therefore allows an absolute
    1e-12 times the largest magnitude of the compared block (the form of test_reference_shapes_gpu.py), which for entries much
    smaller than that maximum is looser than a plain relative 1e-12.  The same holds for the resident-against-host comparison
    of test_hip_resident_sine_trajectory_with_fourteen_pair_costs (two launch sequences of the same kernels)."""
    table, po, ref, x0, xs, us = _panda_problem()
    out = {}
    for wide in ("0", "1"):
        monkeypatch.setenv("AGX_COST_WIDE", wide)
        h = hip_backend.HipOcp(table, po, B)
        h.set_refs(ref)
        h.upload_warmstart(xs, us)
        q, a = h.qp_tiles()
        out[wide] = (q, a, h.solve(x0, xs, us, 30))
        if wide == "1":  # such a handle takes no frame-id table
            with pytest.raises(hip_backend.HipError, match="no frame-id table"):
                h.set_refs(ref, po.default_frames(B))
        h.close()
    (q0, a0, r0), (q1, a1, r1) = out["0"], out["1"]
    for name in q0:
        scale = np.abs(q0[name]).max()
        np.testing.assert_allclose(q1[name], q0[name], rtol=1e-12, atol=1e-12 * scale, err_msg=name)
    np.testing.assert_allclose(a1["Lqq"], a0["Lqq"], rtol=1e-12, atol=1e-12 * np.abs(a0["Lqq"]).max())
    for key in ("iter", "solved", "flags"):
        assert np.array_equal(r0[3][key], r1[3][key]), key
    for i in range(3):
        np.testing.assert_allclose(r1[i], r0[i], rtol=1e-12, atol=1e-12 * max(np.abs(r0[i]).max(), 1.0))
    # against the checker: the tolerances of the full solves of test_model_sizes.py
    xs_o, us_o, K_o, st_o = _oracle(table, po).solve(ref, None, x0, xs, us, 30)
    assert np.array_equal(r1[3]["iter"], st_o["iter"]) and np.array_equal(r1[3]["solved"], st_o["solved"])
    np.testing.assert_allclose(r1[0], xs_o, rtol=1e-8, atol=1e-10)
    np.testing.assert_allclose(r1[1], us_o, rtol=1e-8, atol=1e-8)
    assert np.abs(r1[2] - K_o).max() / np.abs(K_o).max() < 1e-7


@pytest.mark.gpu
@pytest.mark.parametrize("n", [24, 64])
def test_hip_full_solve_with_pair_costs_matches_the_checker_and_repeats_bitwise(hip_backend, n):
    """T = 10, 30 iterations: identical SQP iteration counts and solved flags, xs / us to 1e-8, K to 1e-7 (the stated tolerances of
    test_model_sizes.py); the same solve twice in one process gives bitwise equal results."""
    table, po, ref, x0, xs, us, (xs_o, us_o, K_o, st_o) = _checker_solve(n)
    h = hip_backend.HipOcp(table, po, B)
    h.set_refs(ref)
    xs_h, us_h, K_h, st_h = h.solve(x0, xs, us, 30)
    print("iter", st_h["iter"], st_o["iter"], "flags", st_h["flags"], st_o["flags"])
    print("xs", np.abs(xs_h - xs_o).max(), "us", np.abs(us_h - us_o).max(), "K", np.abs(K_h - K_o).max() / np.abs(K_o).max())
    assert np.array_equal(st_h["iter"], st_o["iter"]) and np.array_equal(st_h["solved"], st_o["solved"])
    np.testing.assert_allclose(xs_h, xs_o, rtol=1e-8, atol=1e-10)
    np.testing.assert_allclose(us_h, us_o, rtol=1e-8, atol=1e-8)
    assert np.abs(K_h - K_o).max() / np.abs(K_o).max() < 1e-7
    again = h.solve(x0, xs, us, 30)
    for a, b_ in zip(again[:3], (xs_h, us_h, K_h)):
        np.testing.assert_array_equal(a, b_)
    h.close()


@pytest.mark.gpu
def test_hip_resident_sine_trajectory_with_fourteen_pair_costs(hip_backend):
    """agx_traj_get_tile shows the pair rows' weights; three resident MPC steps equal the same steps driven with host tiles and
    shift_warmstart to 1e-12."""
    table = _chain()
    T, n, n_points = 10, 14, 16
    po, ref, x0, xs, us = _problem(table, n, T=T)
    tool = table.frame_id("tool")
    q0, amp, puls, scale, t0 = workloads.sine_batch_params(B, nv=6, q0=np.zeros(6))
    w = dict(w_q=np.full(6, 1.0), w_qdot=np.full(6, 0.1), w_effort=np.full(6, 1e-3), w_pose=np.full(6, 2.0))
    h = hip_backend.HipOcp(table, po, B)
    h.sine_trajectory(n_points, 0.01, q0, amp, puls, scale, t0, w["w_q"], w["w_qdot"], w["w_effort"], w["w_pose"], tool)
    tiles = np.stack([h.traj_tile(k) for k in range(n_points)], axis=1)
    tiles_t = np.stack([h.traj_tile(k, terminal=True) for k in range(n_points)], axis=1)
    assert tiles.shape == (B, n_points, po.stride)
    for p in range(n):
        o_r, o_t = po.running_offsets[3 + p], po.terminal_offsets[2 + p]
        assert np.all(tiles[..., o_r] == 0.1) and np.all(tiles[..., o_r + 1] == 1.0)
        assert np.all(tiles_t[..., o_t] == 0.1) and np.all(tiles_t[..., o_t + 1] == 1.0)
    g = hip_backend.HipOcp(table, po, B)  # the same steps with host tiles
    for k in range(3):
        h.mpc_step(k, 10, first=(k == 0))
        r_h = h.download()
        host = np.concatenate([tiles[:, k:k + T], tiles_t[:, k + T:k + T + 1]], axis=1)
        g.set_refs(host)
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
def test_hip_resident_cartesian_trajectory_fills_the_pair_rows(hip_backend):
    """The Cartesian generator on a wide cost set: the pair rows of every sample hold [item weight | 1], as those of the sine
    generator above.  Amplitude 0: every target is the initial pose, so the inverse kinematics has nothing to do."""
    table = _chain()
    T, n, n_points = 4, 14, 6
    po, *_ = _problem(table, n, T=T)
    h = hip_backend.HipOcp(table, po, B)
    q0 = np.tile(np.array([0.1, -0.4, 0.3, -0.8, 0.2, 0.5]), (B, 1))
    h.cartesian_sine_trajectory(n_points, 0.01, q0, np.zeros((B, 3)), np.ones((B, 3)), np.full(6, 1.0), np.full(6, 0.1), np.full(6, 1e-3),
                                np.full(6, 2.0), table.frame_id("tool"))
    tiles = np.stack([h.traj_tile(k) for k in range(n_points)], axis=1)
    tiles_t = np.stack([h.traj_tile(k, terminal=True) for k in range(n_points)], axis=1)
    for p in range(n):
        o_r, o_t = po.running_offsets[3 + p], po.terminal_offsets[2 + p]
        assert np.all(tiles[..., o_r] == 0.1) and np.all(tiles[..., o_r + 1] == 1.0)
        assert np.all(tiles_t[..., o_t] == 0.1) and np.all(tiles_t[..., o_t + 1] == 1.0)
    np.testing.assert_allclose(h.traj_point(n_points - 1)[0], q0, atol=1e-12)
    h.close()


@pytest.mark.gpu
def test_hip_pair_costs_next_to_a_wide_constraint_set_match_the_checker(hip_backend):
    """14 pair costs next to a state box, torque limits and 12 pair constraints (wide constraint layout); the tolerances of
    test_many_collision_pairs.py::_assert_matches_checker."""
    table = _chain()
    run, term = _rows(table, 14)
    lim = np.asarray(table.effort_limit, dtype=float)
    con = [_abi.ConstraintSpec(_abi.RES_STATE, lower=-5.0, upper=5.0, name="box"),
           _abi.ConstraintSpec(_abi.RES_CONTROL, lower=-lim, upper=lim, name="torque")]
    con += workloads.collision_pair_constraints(table, _pairs(16)[4:], 0.01)
    po = _abi.PackedOcp(6, [0.01] * 10, run, term, max_qp_iters=100, running_constraints=con, terminal_constraints=con)
    _, ref, x0, xs, us = _problem(table, 14)
    h, o = hip_backend.HipOcp(table, po, B), _oracle(table, po)
    h.set_refs(ref)
    r_o = o.solve(ref, None, x0, xs, us, 2)
    r_h = h.solve(x0, xs, us, 2)
    assert np.array_equal(r_h[3]["qp_iters"], r_o[3]["qp_iters"])
    np.testing.assert_allclose(r_h[0], r_o[0], rtol=1e-7, atol=1e-8)
    np.testing.assert_allclose(r_h[1], r_o[1], rtol=1e-6, atol=1e-6)
    np.testing.assert_allclose(r_h[2], r_o[2], rtol=1e-5, atol=1e-5)
    np.testing.assert_allclose(r_h[3]["kkt"], r_o[3]["kkt"], rtol=1e-5, atol=1e-8)
    h.close()


def _create_fails(backend, table, po):
    """agx_ocp_create through the C ABI: the return code, the message it leaves and the handle it must not hand out."""
    L = backend.lib()
    pm = _abi.PackedModel(table)
    m, hdl = C.c_void_p(), C.c_void_p()
    assert L.agx_model_create(C.byref(pm.desc), C.byref(m)) == 0
    rc = L.agx_ocp_create(m, C.byref(po.desc), 1, 0, C.byref(hdl))
    msg = L.agx_last_error().decode()
    L.agx_model_destroy(m)
    assert rc != 0 and not hdl.value
    return msg


@pytest.mark.gpu
def test_hip_refuses_what_a_wide_cost_set_does_not_cover(hip_backend, monkeypatch):
    table = _chain()
    run, term = _rows(table, 64)
    monkeypatch.setattr(_abi, "check_cost_rows", lambda *args, **kwargs: None)
    extra = workloads.collision_pair_costs(table, [("cap5", "ob11")])
    assert "at most 64" in _create_fails(hip_backend, table, _abi.PackedOcp(6, [0.01] * 4, run + extra, term))
    other = [_abi.RowSpec(_abi.RES_STATE, name=f"s{i}") for i in range(9)]
    assert "at most 8" in _create_fails(hip_backend, table, _abi.PackedOcp(6, [0.01] * 4, other + run[3:], term))
    assert "trailing rows" in _create_fails(hip_backend, table, _abi.PackedOcp(6, [0.01] * 4, run[3:12] + run[:3], term))
    for base, word in ((rt.tree_table(6, seed=3), "trees"), (rt.chain_table(9, seed=4), "7 joints")):
        t = base
        for j in range(1, 6):
            t = t.with_geometry(f"cap{j}", j, rt.se3(None, [0.0, 0.0, 0.05]), 0.04, 0.06)
        t = t.with_geometry("ob0", -1, rt.se3(None, [0.6, 0.1, 0.3]), 0.05, 0.0)
        r2, t2 = workloads.regulation_rows()
        pc = workloads.collision_pair_costs(t, [(c, "ob0") for c in CAPS] * 2)
        assert word in _create_fails(hip_backend, t, _abi.PackedOcp(t.nv, [0.01] * 4, list(r2) + pc, list(t2)))
    # a frame-id table on a wide handle
    po, ref, *_ = _problem(table, 9, T=4)
    h = hip_backend.HipOcp(table, po, B)
    with pytest.raises(hip_backend.HipError, match="no frame-id table"):
        h.set_refs(ref, po.default_frames(B))
    h.set_refs(ref)  # and the handle is still good
    h.close()


def _generic_yaml(n_pairs):
    """The goal-reaching items of ocp_goal_reaching.yaml on the chain's tool frame plus n_pairs collision cost items, last."""
    quad = {"class": "ActivationModelWeightedQuad", "weights": 1.0}
    item = lambda name, res: {"name": name, "update": True, "weight": 1.0,  # noqa: E731
                              "cost": {"class": "CostModelResidual", "residual": res, "activation": quad}}
    coll = [{"name": f"collision_{i}", "update": True, "weight": 0.1,
             "cost": {"class": "CostModelResidual", "activation": {"class": "ActivationModelQuadExp", "alpha": 0.05},
                      "residual": {"class": "ResidualDistanceCollision", "collision_pair_id": i}}} for i in range(n_pairs)]
    goal = item("goal_tracking", {"class": "ResidualModelFramePlacement", "id": "tool"})
    state = item("state_reg", {"class": "ResidualModelState"})
    model = lambda costs: {"class": "IntegratedActionModelEuler",  # noqa: E731
                           "differential": {"class": "DifferentialActionModelFreeFwdDynamics", "costs": costs}}
    return {"running_model": model([item("control_reg", {"class": "ResidualModelControl"}), state, goal] + coll),
            "terminal_model": model([state, goal] + coll)}


@pytest.mark.gpu
def test_hip_ocp_croco_generic_with_twelve_collision_cost_items(hip_backend):
    """The class surface on a wide cost set: OCPCrocoGeneric from a YAML with 3 + 12 cost items, set_reference_weighted_trajectory
    (w_collision_avoidance reaches every pair row) and a solve equal to the checker's on the same tile; a trajectory point that
    asks for another frame than the item's own is refused with a ValueError."""
    import io

    import yaml

    from agimus_controller_amd import se3
    from agimus_controller_amd.factory.robot_model import RobotModelParameters, RobotModels
    from agimus_controller_amd.ocp.ocp_croco_generic import OCPCrocoGeneric
    from agimus_controller_amd.ocp_param_base import DTFactorsNSeq, OCPParamsBaseCroco
    from agimus_controller_amd.trajectory import TrajectoryPoint, TrajectoryPointWeights, WeightedTrajectoryPoint

    table, T, n = _chain(), 8, 12
    q0 = np.array([0.2, -0.3, 0.4, 0.1, -0.2, 0.3])
    rm = RobotModels(RobotModelParameters(table=table, armature=table.armature, q0=q0, collision_pairs=_pairs(n)))
    params = OCPParamsBaseCroco(dt=0.01, horizon_size=T, dt_factor_n_seq=DTFactorsNSeq(factors=[1], n_steps=[T]), solver_iters=20, callbacks=False)
    ocp = OCPCrocoGeneric(rm, params, io.StringIO(yaml.safe_dump(_generic_yaml(n))))
    assert ocp._hip.cost_wide and ocp.problem.desc.n_running_rows == 3 + n and ocp.problem.desc.n_terminal_rows == 2 + n
    start = ocp._hip.frame_placement(table.frame_id("tool"), q0)[0]
    goal = se3.SE3(start[:9].reshape(3, 3), start[9:] + np.array([0.05, -0.04, 0.03]))

    def point(frame, w_coll):
        return WeightedTrajectoryPoint(
            TrajectoryPoint(robot_configuration=q0, robot_velocity=np.zeros(6), robot_effort=np.zeros(6), end_effector_poses={frame: goal}),
            TrajectoryPointWeights(w_robot_configuration=0.01 * np.ones(6), w_robot_velocity=0.1 * np.ones(6), w_robot_effort=1e-4 * np.ones(6),
                                   w_end_effector_poses={frame: 20.0 * np.ones(6)}, w_collision_avoidance=w_coll))

    ocp.set_reference_weighted_trajectory([point("tool", 0.5 + 0.1 * t) for t in range(T + 1)])
    po = ocp.problem
    for p in range(n):
        np.testing.assert_array_equal(po.row_view(ocp._ref_tile, False, 3 + p)[0][0], 0.5 + 0.1 * np.arange(T))
        np.testing.assert_array_equal(po.row_view(ocp._ref_tile, True, 2 + p)[0][0], [0.5 + 0.1 * T])
    x0 = np.concatenate([q0, np.zeros(6)])
    ocp.solve(x0, [x0] * (T + 1), [np.zeros(6)] * T)
    xs, us = np.array(ocp.ocp_results.states), np.array(ocp.ocp_results.feed_forward_terms)
    xs_o, us_o, K_o, st_o = _oracle(table, po, 1).solve(ocp._ref_tile, None, x0[None], np.tile(x0, (1, T + 1, 1)), np.zeros((1, T, 6)), 20)
    assert ocp._last_status["iter"][0] == st_o["iter"][0] and ocp._last_status["solved"][0] == st_o["solved"][0]
    np.testing.assert_allclose(xs, xs_o[0], rtol=1e-8, atol=1e-10)
    np.testing.assert_allclose(us, us_o[0], rtol=1e-8, atol=1e-8)
    # the pair rows shape it: with their weight at zero the solve ends elsewhere
    ocp.set_reference_weighted_trajectory([point("tool", 0.0)] * (T + 1))
    ocp.solve(x0, [x0] * (T + 1), [np.zeros(6)] * T)
    assert np.abs(np.array(ocp.ocp_results.states) - xs).max() > 1e-6
    with pytest.raises(ValueError, match="goal_tracking.*per-node frame ids are not supported"):
        ocp.set_reference_weighted_trajectory([point("joint3", 1.0)] * (T + 1))
