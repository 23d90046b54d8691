"""Per-item cost values and gradients (agx_ocp_item_costs): what the MPC debugger reads out of Crocoddyl's
cost data.  Every item is checked against a checker that holds that row alone -- the CPU checker, or tests/joint_ref.py for
models with prismatic joints -- on that row's slice of the reference tile: item x dt[t] on the running nodes and the plain item
on the terminal node are the cost, Lx and Lu of the single-row tiles, and the items of a node sum to agx_ocp_calc_diff."""
import numpy as np
import pytest

import joint_ref as jr
import test_general_rows as general
import test_many_collision_costs as mcc
import test_model_sizes as sizes
import test_prismatic_gpu as prismatic
from agimus_controller_amd import _abi, workloads
from agimus_controller_amd.factory import robot_tables as rt
from oracle.oracle import Oracle

pytestmark = pytest.mark.gpu

TS = [0.01, 0.01, 0.02, 0.02]  # mixed dt, T = 4
TOL7, TOL16 = 1e-11, 1e-10  # the project's tile tolerances: models of at most 7 joints / the 16-joint capacity


def _single_row_tiles(tables, po, ref, frames, xs, us, terminal, r, use_joint_ref=False):
    """Canonical tiles [B][T+1][tile] of the problem that holds row r of one node type alone, on that row's slice of the tile.
    tables: one robot table, or one per instance (per-instance worlds)."""
    B, T, nv = xs.shape[0], po.horizon, po.nv
    row = (po.terminal if terminal else po.running)[r]
    off = (po.terminal_offsets if terminal else po.running_offsets)[r]
    one = _abi.PackedOcp(nv, po.dt, [] if terminal else [row], [row] if terminal else [])
    assert one.stride == row.width(nv)
    ref1 = np.zeros((B, T + 1, one.stride))
    nodes = slice(T, T + 1) if terminal else slice(0, T)
    ref1[:, nodes] = ref[:, nodes, off:off + one.stride]
    fr1 = None
    if frames is not None:
        fr1 = np.full((B, T + 1, _abi.AGX_MAX_ROWS), -1, dtype=np.int32)
        fr1[:, nodes, 0] = frames[:, nodes, r]
    if use_joint_ref:
        assert fr1 is None
        return jr.calc_diff(tables, one, ref1, xs, us)
    if not isinstance(tables, list):
        return Oracle(tables, one, B).calc_diff(ref1, fr1, xs, us)
    return np.concatenate([Oracle(tables[b], one, 1).calc_diff(ref1[b:b + 1], None if fr1 is None else fr1[b:b + 1], xs[b:b + 1], us[b:b + 1])
                           for b in range(B)])


EPS = np.finfo(float).eps


def _close(got, want, tol, what, floor=0.0):
    """The project's tile form: |got - want| <= tol x the largest entry of that field (of the checker's).  floor: see _check_items."""
    err, scale = float(np.abs(got - want).max()), float(np.abs(want).max())
    print(f"{what}: err {err:.3e} scale {scale:.3e} floor {floor:.1e}")
    assert err <= tol * scale + floor, what


def _check_items(h, tables, po, ref, frames, xs, us, tol, use_joint_ref=False, rows=None):
    """Every item (or the items `rows` = (running, terminal) index lists) against its single-row checker; the sum against
    calc_diff.  Returns the items."""
    B, T, nv = xs.shape[0], po.horizon, po.nv
    nx = 2 * nv
    sl = _abi.tile_slices(nv)
    it = h.item_costs()
    Rr, Rt = len(po.running), len(po.terminal)
    assert it["cost_r"].shape == (B, T, Rr) and it["Lx_r"].shape == (B, T, Rr, nx) and it["Lu_r"].shape == (B, T, Rr, nv)
    assert it["cost_t"].shape == (B, Rt) and it["Lx_t"].shape == (B, Rt, nx)
    dt = np.asarray(po.dt)[None, :, None]
    for terminal, idx in ((False, range(Rr) if rows is None else rows[0]), (True, range(Rt) if rows is None else rows[1])):
        for r in idx:
            row = (po.terminal if terminal else po.running)[r]
            want = _single_row_tiles(tables, po, ref, frames, xs, us, terminal, r, use_joint_ref)
            if terminal:
                got = (it["cost_t"][:, r], it["Lx_t"][:, r], np.zeros((B, nv)))
                want = (want[:, T, sl["cost"]][:, 0], want[:, T, sl["Lx"]], want[:, T, sl["Lu"]])
            else:
                got = (it["cost_r"][:, :, r] * dt[..., 0], it["Lx_r"][:, :, r] * dt, it["Lu_r"][:, :, r] * dt)
                want = (want[:, :T, sl["cost"]][..., 0], want[:, :T, sl["Lx"]], want[:, :T, sl["Lu"]])
            # Every field against its own largest entry.  A field that is an exact zero on the device (Lx of a Control row, Lu of a
            # State row) may carry the rounding noise of the checker's automatic differentiation: at most one unit of round-off
            # of the item's largest entry, the absolute floor -- five orders below tol x any field that is not zero.
            largest = max(float(np.abs(w).max()) for w in want)
            if row.active and not (terminal and row.kind in (_abi.RES_CONTROL, _abi.RES_CONTROL_GRAV)):
                assert largest > 1e-12, f"item {row.name}: the case evaluates it to nothing"
            for name, g, w in zip(("cost", "Lx", "Lu"), got, want):
                _close(g, w, tol, f"{'terminal' if terminal else 'running'} item {r} ({row.name}) {name}", floor=EPS * largest)
    tiles = h.calc_diff()
    for name, run, term in (("cost", it["cost_r"].sum(2)[..., None] * dt, it["cost_t"].sum(1)[:, None]),
                            ("Lx", it["Lx_r"].sum(2) * dt, it["Lx_t"].sum(1)), ("Lu", it["Lu_r"].sum(2) * dt, np.zeros((B, nv)))):
        want = tiles[..., sl[name]]
        got = np.concatenate([run, term[:, None, :]], axis=1)
        _close(got, want, tol, f"sum of the items x dt against calc_diff: {name}")
    return it


def _chain6_rows(table):
    """Eight rows on the 6-joint chain of tests/test_many_collision_costs.py: quadratic, vector Exp and vector QuadExp activations
    on State / translation / rotation / placement residuals, and collision rows capsule / capsule, capsule / sphere, capsule / box."""
    tool = table.frame_id("tool")
    fid = table.frame_id
    running = [_abi.RowSpec(_abi.RES_CONTROL, name="control_reg"),
               _abi.RowSpec(_abi.RES_STATE, activation=_abi.ACT_EXP, alpha=3.0, name="state_exp"),
               _abi.RowSpec(_abi.RES_FRAME_TRANSLATION, frame=tool, name="translation"),
               _abi.RowSpec(_abi.RES_FRAME_ROTATION, frame=tool, activation=_abi.ACT_QUAD_EXP, alpha=4.0, name="rotation_quadexp"),
               _abi.RowSpec(_abi.RES_FRAME_PLACEMENT, frame=tool, activation=_abi.ACT_EXP, alpha=2.0, name="placement_exp"),
               _abi.RowSpec(_abi.RES_COLLISION, activation=_abi.ACT_QUAD_EXP, alpha=0.5, frame=fid("cap1"), frame_b=fid("cap4"), name="capsule_capsule"),
               _abi.RowSpec(_abi.RES_COLLISION, activation=_abi.ACT_EXP, alpha=0.5, frame=fid("cap5"), frame_b=fid("ob1"), name="capsule_sphere"),
               _abi.RowSpec(_abi.RES_COLLISION, activation=_abi.ACT_QUAD_EXP, alpha=0.5, frame=fid("cap3"), frame_b=fid("ob2"), name="capsule_box")]
    return running, running[1:]


def _case(name):
    """(table, po, ref, xs, us, tol, use_joint_ref) of a parametrised case; B = 2 or 3, T = 4 with mixed dt."""
    if name == "panda":
        table = rt.panda_table(0.1)
        po, ref, _, xs, us = workloads.random_goal_problem(table, 4, 0.01, 2, seed=3, frame=table.frame_id("panda_hand_tcp"), timesteps=TS)
        return table, po, ref, xs, us, TOL7, False
    if name == "chain6_exp_collision":
        table = mcc._chain()
        po, ref, _, xs, us = workloads.random_goal_problem(table, 4, 0.01, 3, seed=7, frame=table.frame_id("tool"), rows=_chain6_rows(table),
                                                           timesteps=TS)
        return table, po, ref, xs, us, TOL7, False
    if name == "control_grav_frame_velocity":
        table = rt.panda_table(0.1)
        po0, ref, _, xs, us = general.general_problem(table, 4, 2, seed=5, ref_frame=1)
        po = _abi.PackedOcp(7, TS, po0.running, po0.terminal)
        return table, po, ref, xs, us, TOL7, False
    if name == "tree6":
        table = rt.tree_table(6, seed=46)
        frame = len(table.frame_names) - 1
        running, terminal = workloads.goal_reaching_rows(frame)
        running = running + [_abi.RowSpec(_abi.RES_FRAME_TRANSLATION, frame=frame - 1, name="second_frame")]
        po, ref, _, xs, us = workloads.random_goal_problem(table, 4, 0.01, 2, seed=9, frame=frame, rows=(running, terminal), timesteps=TS)
        return table, po, ref, xs, us, TOL7, False
    if name == "nine_joints":
        table = sizes._model(9, "panda_fingers")
        po, ref, _, xs, us = workloads.random_goal_problem(table, 4, 0.01, 2, seed=19, frame=len(table.frame_names) - 1, timesteps=TS)
        return table, po, ref, xs, us, TOL16, False
    if name in ("humanoid30", "tree32"):  # the 30- and 32-joint capacities: the tolerance of the canonical tiles of large models
        table = rt.humanoid30_table() if name == "humanoid30" else rt.tree_table(32, seed=72)
        po, ref, _, xs, us = workloads.random_goal_problem(table, 4, 0.01, 2, seed=table.nv, frame=len(table.frame_names) - 1, timesteps=TS)
        return table, po, ref, xs, us, TOL16, False
    assert name == "gantry_prismatic"
    table, tool, _, pair = prismatic.MODELS["gantry7"]
    rows = prismatic._translation_and_collision_rows(tool, pair)
    po, ref, _, xs, us = workloads.random_goal_problem(table, 4, 0.01, 2, seed=47, frame=tool, rows=rows, timesteps=TS)
    return table, po, ref, xs, us, TOL7, True


@pytest.mark.parametrize("name", ["panda", "chain6_exp_collision", "control_grav_frame_velocity", "tree6", "nine_joints", "humanoid30", "tree32",
                                  "gantry_prismatic"])
def test_every_item_against_its_single_row_checker(hip_backend, name):
    table, po, ref, xs, us, tol, use_jr = _case(name)
    h = hip_backend.HipOcp(table, po, xs.shape[0])
    h.set_refs(ref)
    h.upload_warmstart(xs, us)
    it = _check_items(h, table, po, ref, None, xs, us, tol, use_jr)
    # null pointers are skipped
    import ctypes as C

    only = np.empty_like(it["cost_t"])
    assert hip_backend.lib().agx_ocp_item_costs(h._h, None, None, None, only.ctypes.data_as(C.c_void_p), None) == 0
    np.testing.assert_array_equal(only, it["cost_t"])
    h.close()


def test_wide_set_of_three_plus_twelve_pairs_and_per_instance_obstacles(hip_backend):
    """3 + 12 rows: the pair rows come from k_cost_pairs with the per-pair destination.  Then every instance gets its own world."""
    table = mcc._chain()
    run, term = mcc._rows(table, 12)
    po, ref, _, xs, us = workloads.random_goal_problem(table, 5, 0.01, mcc.B, 71, frame=table.frame_id("tool"), rows=(run, term),
                                                       timesteps=[0.01, 0.01, 0.02, 0.02, 0.01])
    assert len(po.running) == 15 and len(po.terminal) == 14
    h = hip_backend.HipOcp(table, po, mcc.B)
    assert h.cost_wide
    h.set_refs(ref)
    h.upload_warmstart(xs, us)
    _check_items(h, table, po, ref, None, xs, us, TOL7)
    obstacles = sorted({b for _, b in mcc._pairs(12) if b.startswith("ob")})
    se3 = workloads.obstacle_placements(table, obstacles, mcc.B, seed=5)
    h.set_obstacle_placements(obstacles, se3)
    worlds = workloads.world_tables(table, obstacles, se3)
    moved = _check_items(h, worlds, po, ref, None, xs, us, TOL7, rows=(range(3, 15), range(2, 14)))
    h.clear_obstacle_placements()
    back = h.item_costs()
    assert not np.array_equal(moved["cost_r"][1:], back["cost_r"][1:])  # the placements matter
    np.testing.assert_array_equal(moved["cost_r"][0], back["cost_r"][0])  # instance 0 keeps the model's
    h.close()


def test_inactive_row_gives_zeros_and_the_frame_table_is_honoured(hip_backend):
    table = rt.panda_table(0.1)
    tcp, other = table.frame_id("panda_hand_tcp"), table.frame_id("panda_hand_tcp") - 1
    running, terminal = workloads.goal_reaching_rows(tcp)
    running[1].active = False
    B, T = 2, 4
    po, ref, _, xs, us = workloads.random_goal_problem(table, T, 0.01, B, seed=21, frame=tcp, rows=(running, terminal), timesteps=TS)
    frames = po.default_frames(B)
    frames[:, 1::2, 2] = other  # the placement row of the running nodes 1 and 3 looks at another frame
    frames[1, T, 1] = other     # ... and that of the terminal node of instance 1
    h = hip_backend.HipOcp(table, po, B)
    h.set_refs(ref, frames)
    h.upload_warmstart(xs, us)
    it = _check_items(h, table, po, ref, frames, xs, us, TOL7)
    assert not it["cost_r"][:, :, 1].any() and not it["Lx_r"][:, :, 1].any() and not it["Lu_r"][:, :, 1].any()
    h.set_refs(ref)
    plain = h.item_costs()
    assert not np.array_equal(plain["cost_r"][:, 1::2, 2], it["cost_r"][:, 1::2, 2])
    np.testing.assert_array_equal(plain["cost_r"][:, 0::2, 2], it["cost_r"][:, 0::2, 2])
    h.close()


def test_item_costs_between_resident_mpc_steps_change_nothing(hip_backend):
    """Four resident MPC steps with item_costs called between them equal the same steps without the call, bit for bit, and as
    many of them inherit the tiles of the step before (carry_counts: a carried and a full step hand out the same bits, the
    count of carried steps is where a call that ended the carry would show)."""
    table = rt.panda_table(0.1)
    tcp = table.frame_id("panda_hand_tcp")
    B, T = 3, 6
    po = _abi.PackedOcp(7, [0.01] * T, *workloads.goal_reaching_rows(tcp), max_qp_iters=100)
    q0, amp, puls, scale, t0 = workloads.sine_batch_params(B, lower=table.lower_position_limit, upper=table.upper_position_limit)
    w = workloads.SINE_WEIGHTS
    runs = []
    for probe in (False, True):
        h = hip_backend.HipOcp(table, po, B)
        h.sine_trajectory(T + 8, 0.01, q0, amp, puls, scale, t0, w["w_q"], w["w_qdot"], w["w_effort"], w["w_pose"], tcp)
        out = []
        for k in range(4):
            h.mpc_step(k, 10, first=(k == 0))
            if probe:
                it = h.item_costs()
                assert np.isfinite(it["cost_r"]).all() and it["cost_r"].any()
            xs, us, K, st = h.download()
            out.append((xs, us, K, np.array(st), h.handoff_counts()[1], h.carry_counts()))
        runs.append(out)
        h.close()
    for k, (a, b) in enumerate(zip(*runs)):
        for name, va, vb in zip(("xs", "us", "K"), a[:3], b[:3]):
            assert np.array_equal(va, vb), f"step {k}: {name}"
        for f in a[3].dtype.names:
            assert np.array_equal(a[3][f], b[3][f], equal_nan=True), f"step {k}: status {f}"
        assert a[4] == b[4], f"step {k}: inheritable instances {a[4]} != {b[4]}"
        assert a[5] == b[5], f"step {k}: (carried, full) steps {a[5]} without the call, {b[5]} with it"
    # the first step starts from the reference, each of the three behind it follows by one sample and carries
    assert runs[0][-1][5] == (3, 1) and runs[1][-1][5] == (3, 1), (runs[0][-1][5], runs[1][-1][5])


def test_item_costs_on_a_window_of_a_resident_trajectory(hip_backend):
    """The references of a resident trajectory's window: the items equal, bit for bit, those of a handle that was given the same
    tiles from the host (traj_tile of every sample of the window) at the same iterate."""
    table = rt.panda_table(0.1)
    tcp = table.frame_id("panda_hand_tcp")
    B, T, k0 = 2, 5, 3
    po = _abi.PackedOcp(7, [0.01] * T, *workloads.goal_reaching_rows(tcp))
    q0, amp, puls, scale, t0 = workloads.sine_batch_params(B, lower=table.lower_position_limit, upper=table.upper_position_limit)
    w = workloads.SINE_WEIGHTS
    h = hip_backend.HipOcp(table, po, B)
    h.sine_trajectory(k0 + T + 4, 0.01, q0, amp, puls, scale, t0, w["w_q"], w["w_qdot"], w["w_effort"], w["w_pose"], tcp)
    h.mpc_step(0, 2, first=True)
    for k in range(1, k0 + 1):
        h.mpc_step(k, 2, first=False)
    resident = h.item_costs()
    xs, us, _, _ = h.download()
    ref = np.stack([h.traj_tile(k0 + t, terminal=(t == T)) for t in range(T + 1)], axis=1)
    h.close()
    assert np.abs(ref[:, :T, po.running_offsets[2] + 1:po.running_offsets[2] + 13]).max() > 0  # the poses of the window
    assert not np.array_equal(ref[:, 0], ref[:, 1])
    g = hip_backend.HipOcp(table, po, B)
    g.set_refs(ref)
    g.upload_warmstart(xs, us)
    host = g.item_costs()
    g.close()
    for name in resident:
        assert np.array_equal(resident[name], host[name]), name
    assert resident["cost_r"].any() and resident["cost_t"].any()


def test_cost_items_of_the_goal_reaching_yaml(hip_backend):
    from agimus_controller_amd.factory.robot_model import panda_robot_models
    from agimus_controller_amd.ocp.ocp_croco_generic import OCPCrocoGeneric
    from agimus_controller_amd.ocp_param_base import DTFactorsNSeq, OCPParamsBaseCroco

    T = 5
    rm = panda_robot_models(0.1)
    params = OCPParamsBaseCroco(dt=0.01, horizon_size=T, dt_factor_n_seq=DTFactorsNSeq([1], [T]), solver_iters=5)
    ocp = OCPCrocoGeneric(rm, params, OCPCrocoGeneric.get_default_yaml_file("ocp_goal_reaching.yaml"))
    from agimus_controller_amd import se3
    from agimus_controller_amd.trajectory import TrajectoryPoint, TrajectoryPointWeights, WeightedTrajectoryPoint

    pt = WeightedTrajectoryPoint(  # the frame item looks at the frame the trajectory point names
        TrajectoryPoint(robot_configuration=workloads.PANDA_Q0, robot_velocity=np.zeros(7), robot_effort=np.zeros(7),
                        end_effector_poses={"panda_hand_tcp": se3.SE3(np.eye(3), np.array([0.5, 0.2, 0.5]))}),
        TrajectoryPointWeights(w_robot_configuration=0.01 * np.ones(7), w_robot_velocity=0.01 * np.ones(7),
                               w_robot_effort=0.0001 * np.ones(7), w_end_effector_poses={"panda_hand_tcp": 10.0 * np.ones(6)}))
    ocp.set_reference_weighted_trajectory([pt] * (T + 1))
    rng = np.random.default_rng(1)
    states = np.concatenate([workloads.PANDA_Q0 + rng.normal(0, 0.05, (T + 1, 7)), rng.normal(0, 0.1, (T + 1, 7))], axis=1)
    controls = rng.normal(0, 1.0, (T, 7))
    out = ocp.cost_items(states, controls)
    assert out.names == ["control_reg", "state_reg", "goal_tracking"]
    assert out.values.shape == (3, T + 1) and out.jacobian.shape == (3, (T + 1) * 21)
    np.testing.assert_array_equal(np.isnan(out.values), [[False] * T + [True], [False] * (T + 1), [False] * (T + 1)])
    it = ocp._hip.item_costs()
    np.testing.assert_array_equal(out.values[:, :T], it["cost_r"][0].T)
    np.testing.assert_array_equal(out.values[1:, T], it["cost_t"][0])
    jac = out.jacobian.reshape(3, T + 1, 21)
    np.testing.assert_array_equal(jac[:, :T, :14], it["Lx_r"][0].transpose(1, 0, 2))
    np.testing.assert_array_equal(jac[:, :T, 14:], it["Lu_r"][0].transpose(1, 0, 2))
    np.testing.assert_array_equal(jac[1:, T, :14], it["Lx_t"][0])
    assert not jac[:, T, 14:].any() and not jac[0, T].any()
    assert np.abs(jac[0, :T, 14:]).max() > 0 and np.abs(jac[2, :, :7]).max() > 0
