"""Prismatic joints on the device, against the numpy reference of tests/joint_ref.py (pinned to the CPU checker on all-revolute
models by tests/test_prismatic.py; the checker itself is revolute only and sees none of these tables).

Models (joint_ref.prismatic_models), the smallest that reach each code path:
  cartpole       nv  2 at capacity  7   one lane per node, a chain demoted to the tree kernels
  gantry7        nv  7 at capacity  7   a serial chain that must NOT take the eight-lane kernels
  panda_gripper  nv  9 at capacity 16   workgroup per node, tree
  tree12p        nv 12 at capacity 16   workgroup per node, tree
  tree30p        nv 30 at capacity 30   workgroup per node, tree
  chain31p       nv 31 at capacity 32   workgroup per node; primitives and derivative tiles only
"""
import os

import numpy as np
import pytest

import joint_ref as jr
from agimus_controller_amd import _abi, workloads
from agimus_controller_amd.factory import robot_tables as rt

pytestmark = pytest.mark.gpu

MODELS = jr.prismatic_models()
ALL = sorted(MODELS)
SOLVED = ["cartpole", "gantry7", "panda_gripper", "tree12p"]
TS = [0.01, 0.01, 0.02, 0.02]


def rel(a, b):
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))


def _translation_and_collision_rows(tool, pair):
    dist = dict(activation=_abi.ACT_QUAD_EXP, alpha=0.05, frame=pair[0], frame_b=pair[1], name="distance")
    running = [_abi.RowSpec(_abi.RES_CONTROL, name="control_reg"), _abi.RowSpec(_abi.RES_STATE, name="state_reg"),
               _abi.RowSpec(_abi.RES_FRAME_TRANSLATION, frame=tool, name="goal_translation"), _abi.RowSpec(_abi.RES_COLLISION, **dist)]
    terminal = [_abi.RowSpec(_abi.RES_STATE, name="state_reg"), _abi.RowSpec(_abi.RES_FRAME_TRANSLATION, frame=tool, name="goal_translation"),
                _abi.RowSpec(_abi.RES_COLLISION, **dist)]
    return running, terminal


@pytest.mark.parametrize("name", ALL)
def test_primitives(hip_backend, name):
    """rnea, frame placement, both frame Jacobian conventions (tool frame and a second frame) and integrate: 1e-11 relative."""
    table, tool, second, _ = MODELS[name]
    nv = table.nv
    po = _abi.PackedOcp(nv, TS, *workloads.goal_reaching_rows(tool))
    h = hip_backend.HipOcp(table, po, 1)
    rng = np.random.default_rng(nv)
    q, v, a = rng.uniform(-1.0, 1.0, (3, 5, nv))
    got, want = h.rnea(q, v, a), jr.rnea(table, q, v, a)
    print(name, "rnea", rel(got, want))
    assert rel(got, want) < 1e-11
    for frame in (tool, second):
        for what, g, w in (("placement", h.frame_placement(frame, q), jr.placement12(table, frame, q)),
                           ("jacobian lwa", h.frame_jacobian(frame, q), jr.frame_jacobian(table, frame, q)),
                           ("jacobian local", h.frame_jacobian(frame, q, local=True), jr.frame_jacobian(table, frame, q, local=True))):
            print(name, frame, what, rel(g, w))
            assert rel(g, w) < 1e-11, (frame, what)
    x = np.concatenate([q, v], 1)
    got, want = h.integrate(x, 3 * a), jr.euler(table, x, 3 * a, TS[0])
    print(name, "integrate", rel(got, want))
    assert rel(got, want) < 1e-11
    h.close()


@pytest.mark.parametrize("rows", ["goal", "translation_collision"])
@pytest.mark.parametrize("name", ALL)
def test_derivative_tiles(hip_backend, name, rows):
    """agx_ocp_calc_diff against the complex-step tiles: State, Control, FramePlacement rows ("goal"), then FrameTranslation and a
    sphere / sphere collision cost row with both spheres below a prismatic joint.  1e-10 of every block."""
    table, tool, _, pair = MODELS[name]
    nv, B, T = table.nv, 3, 4
    rws = "goal" if rows == "goal" else _translation_and_collision_rows(tool, pair)
    po, ref, x0, xs, us = workloads.random_goal_problem(table, T, 0.01, B, seed=40 + nv, frame=tool, rows=rws, timesteps=TS)
    if rows != "goal":
        d = jr.residual(table, _abi.RES_COLLISION, pair[0], pair[1], np.zeros(0), xs, None)
        assert d.min() > 0.02, "the spheres of the test must stay apart"
    h = hip_backend.HipOcp(table, po, B)
    h.set_refs(ref)
    h.upload_warmstart(xs, us)
    got, want = h.calc_diff(), jr.calc_diff(table, po, ref, xs, us)
    assert got.shape == want.shape == (B, T + 1, _abi.tile_doubles(nv))
    for field, s in _abi.tile_slices(nv).items():
        scale = max(np.abs(want[..., s]).max(), 1e-300)
        err = np.abs(got[..., s] - want[..., s]).max()
        print(name, rows, field, err / scale)
        assert err <= 1e-10 * scale, field
    h.close()


@pytest.mark.parametrize("name", [n for n in ALL if n != "chain31p"])
def test_direction(hip_backend, name):
    """h.direction() comes from the acceleration-form tiles of k_calc_qp / k_calc_qp_wg (another kernel than k_calc_diff) and the
    Riccati sweeps: against the dense LQR on the complex-step tiles, to the tolerances of
    tests/test_hip_parity.py::test_direction_kernels_against_oracle."""
    table, tool, _, _ = MODELS[name]
    nv, B, T = table.nv, 2, (4 if name == "tree30p" else 6)
    po, ref, x0, xs, us = workloads.random_goal_problem(table, T, 0.01, B, seed=60 + nv, frame=tool)
    xs[:, 0] = x0
    h = hip_backend.HipOcp(table, po, B)
    h.set_refs(ref)
    h.upload_warmstart(xs, us)
    K, k, dx, du, kkt = h.direction()
    Kr, kr, dxr, dur, kktr = jr.direction(nv, jr.calc_diff(table, po, ref, xs, us))
    print(name, "dx", rel(dx, dxr), "du", rel(du, dur), "K", rel(K, Kr), "kkt", np.abs(kkt / kktr - 1).max())
    assert rel(dx, dxr) < 1e-9 and rel(du, dur) < 1e-9
    assert rel(K, Kr) < 1e-8
    np.testing.assert_allclose(kkt, kktr, rtol=1e-7)
    h.close()


@pytest.mark.parametrize("name", SOLVED)
def test_one_sqp_iteration_replayed(hip_backend, name):
    """solve(max_iter = 1) from a warm start: the helper computes the direction and the merit cost + 10 |gaps|_1 at alpha = 1, 1/2,
    ... and takes the first alpha with merit_try < merit; the returned iterate is xs + alpha dx, us + alpha du."""
    table, tool, _, _ = MODELS[name]
    nv, B, T = table.nv, 2, 6
    po, ref, x0, xs, us = workloads.random_goal_problem(table, T, 0.01, B, seed=80 + nv, frame=tool)
    xs[:, 0] = x0
    h = hip_backend.HipOcp(table, po, B)
    h.set_refs(ref)
    xs_h, us_h, _, st = h.solve(x0, xs, us, 1)
    _, _, dx, du, kkt = jr.direction(nv, jr.calc_diff(table, po, ref, xs, us))
    assert np.all(kkt > 1e-3), "the warm start must not be converged already"
    merit = jr.merit(table, po, ref, xs, us)
    for b in range(B):
        alpha, want_x, want_u = 1.0, xs[b], us[b]
        for _ in range(10):
            tx, tu = xs[b] + alpha * dx[b], us[b] + alpha * du[b]
            if jr.merit(table, po, ref[b : b + 1], tx[None], tu[None])[0] < merit[b]:
                want_x, want_u = tx, tu
                break
            alpha *= 0.5
        print(name, b, "alpha", alpha, "xs", rel(xs_h[b], want_x), "us", rel(us_h[b], want_u))
        assert rel(xs_h[b], want_x) < 1e-8 and rel(us_h[b], want_u) < 1e-8
    h.close()


@pytest.mark.parametrize("name", SOLVED)
def test_full_solve(hip_backend, name):
    """B = 2, T = 20, up to 100 iterations: solved, kkt within the tolerance, the reported cost is the helper's cost of the returned
    trajectory and the helper's dynamics gaps are within the tolerance (they are one of the terms of the KKT measure)."""
    table, tool, _, _ = MODELS[name]
    nv, B, T, tol = table.nv, 2, 20, 1e-3
    po, ref, x0, xs, us = workloads.random_goal_problem(table, T, 0.01, B, seed=90 + nv, frame=tool)
    h = hip_backend.HipOcp(table, po, B)
    h.set_refs(ref)
    xs_h, us_h, _, st = h.solve(x0, xs, us, 100)
    cost = jr.traj_cost(table, po, ref, xs_h, us_h)
    gap = np.abs(jr.gaps(table, po, xs_h, us_h)).max((-1, -2))
    print(name, "iter", st["iter"], "solved", st["solved"], "kkt", st["kkt"], "cost", np.abs(st["cost"] / cost - 1), "gap", gap)
    assert np.all(st["solved"] == 1) and np.all(st["kkt"] <= tol)
    np.testing.assert_array_equal(xs_h[:, 0], x0)
    np.testing.assert_allclose(st["cost"], cost, rtol=1e-9)
    assert np.all(gap <= tol)
    h.close()


def _violation(con, g):
    lo, up = np.broadcast_to(np.asarray(con.lower, dtype=float), g.shape[-1:]), np.broadcast_to(np.asarray(con.upper, dtype=float), g.shape[-1:])
    return float((np.maximum(lo - g, 0.0) + np.maximum(g - up, 0.0)).max())


def test_finger_box_and_torque_limits(hip_backend):
    """panda_gripper: the reference asks the fingers for 0.06 m, their box is 0 ... 0.04 m; torque limits next to it."""
    table, tool, _, _ = MODELS["panda_gripper"]
    nv, B, T, tol = 9, 2, 20, 1e-3
    po0, ref, x0, xs, us = workloads.random_goal_problem(table, T, 0.01, B, seed=7, frame=tool)
    x0[:, 7:9], x0[:, 16:18] = 0.02, 0.0
    xs[:, :, 7:9], xs[:, :, 16:18] = 0.02, 0.0
    for term, row in ((False, 1), (True, 0)):
        wi, rr, aw = po0.row_view(ref, term, row)
        rr[..., 7:9], rr[..., 16:18] = 0.06, 0.0
        aw[..., 7:9] = 200.0
    lo, up = np.full(18, -np.inf), np.full(18, np.inf)
    lo[7:9], up[7:9] = 0.0, 0.04
    box = _abi.ConstraintSpec(_abi.RES_STATE, lower=lo, upper=up, ref=np.zeros(18), name="finger_box")
    ulim = _abi.ConstraintSpec(_abi.RES_CONTROL, lower=-table.effort_limit, upper=table.effort_limit, ref=np.zeros(9), name="torque_limit")
    h0 = hip_backend.HipOcp(table, po0, B)
    h0.set_refs(ref)
    xs_u = h0.solve(x0, xs, us, 100)[0]
    print("unconstrained finger positions up to", xs_u[:, :, 7:9].max())
    assert xs_u[:, :, 7:9].max() > 0.04 + tol  # the box matters: without it the fingers pass it
    h0.close()
    po = _abi.PackedOcp(nv, [0.01] * T, po0.running, po0.terminal, termination_tolerance=tol, max_qp_iters=1000,
                        running_constraints=[box, ulim], terminal_constraints=[box])
    h = hip_backend.HipOcp(table, po, B)
    h.set_refs(ref)
    xs_h, us_h, _, st = h.solve(x0, xs, us, 100)
    viol = max(_violation(box, xs_h), _violation(ulim, us_h))
    print("solved", st["solved"], "iter", st["iter"], "qp_iters", st["qp_iters"], "kkt", st["kkt"], "violation", viol, "fingers up to", xs_h[:, :, 7:9].max())
    assert np.all(st["solved"] == 1)
    assert viol <= tol
    h.close()
    # the position of a fingertip along the solution, through the residual of a FrameTranslation row (reference 0) on a handle
    # that holds the solution: it moves with the prismatic finger joint
    tip = table.frame_id("panda_leftfinger_tip")
    po2 = _abi.PackedOcp(nv, [0.01] * T, po0.running + [_abi.RowSpec(_abi.RES_FRAME_TRANSLATION, frame=tip, name="fingertip")], po0.terminal)
    h2 = hip_backend.HipOcp(table, po2, B)
    h2.set_refs(po2.new_ref_tile(B))
    h2.upload_warmstart(xs_h, us_h)
    got, want = h2.residuals(3), jr.residual(table, _abi.RES_FRAME_TRANSLATION, tip, 0, np.zeros(3), xs_h[:, :T], None)
    assert rel(got, want) < 1e-11
    h2.close()


def test_translation_bound_along_a_prismatic_joint(hip_backend):
    """gantry7: the state reference sends prismatic joint 0 away by 0.6 m, which carries the tool along the joint's (constant) world
    axis z; a FrameTranslation bound stops the tool 0.15 m down that way, on the world coordinate z is most aligned with."""
    table, tool, _, _ = MODELS["gantry7"]
    nv, B, T, dt, tol = 7, 2, 20, 0.05, 1e-3
    rows = ([_abi.RowSpec(_abi.RES_CONTROL, name="control_reg"), _abi.RowSpec(_abi.RES_STATE, name="state_reg"),
             _abi.RowSpec(_abi.RES_FRAME_TRANSLATION, frame=tool, name="tool_translation")],
            [_abi.RowSpec(_abi.RES_STATE, name="state_reg"), _abi.RowSpec(_abi.RES_FRAME_TRANSLATION, frame=tool, name="tool_translation")])
    po0, ref, x0, xs, us = workloads.random_goal_problem(table, T, dt, B, seed=12, frame=tool, rows=rows)
    x0[:, nv:] = 0.0
    xs[:] = x0[:, None, :]
    us[:] = jr.rnea(table, x0[:, :nv], 0.0 * x0[:, :nv], 0.0 * x0[:, :nv])[:, None, :]
    p0 = jr.frame_placement(table, tool, x0[:, :nv])[1]
    for term, srow, trow in ((False, 1, 2), (True, 0, 1)):
        wi, rr, aw = po0.row_view(ref, term, srow)
        rr[..., :nv], rr[..., nv:] = x0[:, None, :nv], 0.0
        rr[..., 0] += 0.6
        aw[..., 0] = 50.0
        wi, rr, aw = po0.row_view(ref, term, trow)
        wi[...] = 1e-3
        rr[...] = p0[:, None, :]
    z = np.asarray(table.placement[0][:9]).reshape(3, 3) @ table.axis[0]  # joint 0 is a root joint: its world axis is constant
    e = int(np.argmax(np.abs(z)))
    lo, up = np.full(3, -np.inf), np.full(3, np.inf)
    if z[e] > 0.0:
        up[e] = 0.15 * abs(z[e])
    else:
        lo[e] = -0.15 * abs(z[e])
    h0 = hip_backend.HipOcp(table, po0, B)
    h0.set_refs(ref)
    xs_u, _, _, st_u = h0.solve(x0, xs, us, 100)
    h0.close()
    worst, solved = [], []
    for b in range(B):  # the bound is relative to the tool position of the instance at x0
        con = _abi.ConstraintSpec(_abi.RES_FRAME_TRANSLATION, lower=lo, upper=up, ref=p0[b], frame=tool, name="tool_stop")
        r_u = jr.residual(table, _abi.RES_FRAME_TRANSLATION, tool, 0, p0[b], xs_u[b], None)
        print("instance", b, "unconstrained violation", _violation(con, r_u), "solved", st_u["solved"][b])
        assert _violation(con, r_u) > 100 * tol
        po = _abi.PackedOcp(nv, [dt] * T, po0.running, po0.terminal, termination_tolerance=tol, max_qp_iters=1000,
                            running_constraints=[con], terminal_constraints=[con])
        h = hip_backend.HipOcp(table, po, 1)
        h.set_refs(ref[b : b + 1])
        xs_h, us_h, _, st = h.solve(x0[b : b + 1], xs[b : b + 1], us[b : b + 1], 100)
        r = jr.residual(table, _abi.RES_FRAME_TRANSLATION, tool, 0, p0[b], xs_h[0], None)
        print("instance", b, "solved", st["solved"], "iter", st["iter"], "qp_iters", st["qp_iters"], "kkt", st["kkt"], "violation", _violation(con, r))
        solved.append(int(st["solved"][0]))
        worst.append(_violation(con, r))
        want = jr.residual(table, _abi.RES_FRAME_TRANSLATION, tool, 0, po.row_view(ref[b : b + 1], False, 2)[1], xs_h[:, :T], None)
        assert rel(h.residuals(2), want) < 1e-11
        h.close()
    assert solved == [1] * B
    assert max(worst) <= tol


def _sine(h, table, tool, n_points, dt):
    nv, B = table.nv, h.B
    q0 = np.tile(np.concatenate([workloads.PANDA_Q0, [0.02, 0.02]]) if nv == 9 else np.zeros(nv), (B, 1)) + 0.01 * np.arange(B)[:, None]
    amp = np.full((B, nv), 0.1)
    if nv == 9:
        amp[:, 7:] = 0.01
    puls = np.full((B, nv), 2.0 * np.pi / 4.0)
    w = workloads.SINE_WEIGHTS
    h.sine_trajectory(n_points, dt, q0, amp, puls, np.full((B, nv), 0.2), 0.5 * np.arange(B), w["w_q"], w["w_qdot"], w["w_effort"], w["w_pose"], tool)


def test_resident_mpc_loop_on_the_gripper(hip_backend):
    """sine_trajectory + 4 mpc_steps: the generated points go through kinematics() / rnea() on the device."""
    table, tool, _, _ = MODELS["panda_gripper"]
    B, T, dt = 2, 10, 0.01
    po = _abi.PackedOcp(9, [dt] * T, *workloads.goal_reaching_rows(tool))
    h = hip_backend.HipOcp(table, po, B)
    _sine(h, table, tool, T + 8, dt)
    o = po.running_offsets[2]
    for k in (0, 3, T + 2):
        q, v, a, u, pose = h.traj_point(k)
        want = jr.placement12(table, tool, q)
        assert np.abs(q[:, 7:]).max() > 0.0
        assert rel(pose, want) < 1e-11
        assert rel(h.traj_tile(k)[:, o + 1 : o + 13], want) < 1e-11
        assert rel(u, jr.rnea(table, q, v, a)) < 1e-10
    for k in range(4):
        h.mpc_step(k, 10, first=(k == 0))
        st = h.download_first()[3]
        print("step", k, "solved", st["solved"], "iter", st["iter"])
        assert np.all(st["solved"] == 1)
    h.close()


def test_tile_carry_stays_off_for_a_chain_with_prismatic_joints(hip_backend):
    """gantry7 is a serial chain, but not one of revolute joints: the tile carry (a feature of the eight-lane path) must be off, so
    AGX_TILE_CARRY changes nothing -- 4 MPC steps are bitwise equal (the switch is read when a handle is created)."""
    table, tool, _, _ = MODELS["gantry7"]
    B, T, dt = 2, 10, 0.01
    po = _abi.PackedOcp(7, [dt] * T, *workloads.goal_reaching_rows(tool))
    runs = []
    for carry in ("0", "1"):
        old = os.environ.get("AGX_TILE_CARRY")
        os.environ["AGX_TILE_CARRY"] = carry
        try:
            h = hip_backend.HipOcp(table, po, B)
        finally:
            if old is None:
                del os.environ["AGX_TILE_CARRY"]
            else:
                os.environ["AGX_TILE_CARRY"] = old
        _sine(h, table, tool, T + 8, dt)
        out = []
        for k in range(4):
            h.mpc_step(k, 10, first=(k == 0))
            xs, us, K, st = h.download()
            out.append((xs, us, K, np.array(st)))
        runs.append(out)
        h.close()
    for k, (a, b) in enumerate(zip(*runs)):
        assert np.all(a[3]["solved"] == 1), k
        for name, va, vb in zip(("xs", "us", "K"), a[:3], b[:3]):
            assert np.array_equal(va, vb), f"step {k}: {name} differs"
        for field in a[3].dtype.names:
            assert np.array_equal(a[3][field], b[3][field], equal_nan=True), f"step {k}: status word {field} differs"


def test_refusals(hip_backend):
    table, tool, _, pair = MODELS["gantry7"]
    po = _abi.PackedOcp(7, TS, *workloads.goal_reaching_rows(tool))
    bad = jr.with_prismatic(table, [0, 3])
    bad.joint_type[1] = 2
    with pytest.raises(hip_backend.HipError, match="joint 1 has joint_type 2"):
        hip_backend.HipOcp(bad, po, 1)
    running, terminal = workloads.goal_reaching_rows(tool)
    wide = running + workloads.collision_pair_costs(table, [pair] * 6)
    assert len(wide) > _abi.AGX_MAX_ROWS
    with pytest.raises(hip_backend.HipError, match="serial chain of revolute joints"):
        hip_backend.HipOcp(table, _abi.PackedOcp(7, TS, wide, terminal), 1)
    # the same set on the same chain with revolute joints only is a wide cost set
    h = hip_backend.HipOcp(rt.chain_table(7, seed=3).with_geometry("sphere_a", 6, rt.se3(None, [0.02, 0.0, 0.03]), radius=0.02)
                           .with_geometry("sphere_b", 3, rt.se3(None, [0.0, -0.03, 0.01]), radius=0.02), _abi.PackedOcp(7, TS, wide, terminal), 1)
    assert h.cost_wide
    h.close()
