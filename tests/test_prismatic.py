"""Prismatic joints, the part that needs no GPU: the numpy reference of tests/joint_ref.py pinned to the golden-pinned CPU
checker on all-revolute models (the checker is revolute only: no table with a prismatic joint ever goes there), then used on
closed forms with prismatic joints, and the host layers that carry the joint type."""
import ctypes as C
import dataclasses

import numpy as np
import pytest

import joint_ref as jr
from agimus_controller_amd import _abi, workloads
from agimus_controller_amd.factory import robot_tables as rt
from oracle import oracle as orc
from oracle.oracle import Oracle


def rel(a, b):
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))


REVOLUTE = {"chain7": lambda: rt.chain_table(7, seed=3), "tree12": lambda: rt.tree_table(12, seed=52)}
TS = [0.01, 0.01, 0.02, 0.02]


@pytest.fixture(scope="module", params=sorted(REVOLUTE))
def pinned(request):
    """One all-revolute model with the goal problem, the checker's tiles and the helper's tiles at the same point."""
    table = REVOLUTE[request.param]()
    B, T = 3, 4
    po, ref, x0, xs, us = workloads.random_goal_problem(table, T, 0.01, B, seed=17, frame=len(table.frame_names) - 1, timesteps=TS)
    xs[:, 0] = x0
    o = Oracle(table, po, B)
    return table, po, ref, xs, us, o, o.calc_diff(ref, None, xs, us), jr.calc_diff(table, po, ref, xs, us)


def test_helper_rnea_and_frames_match_the_checker(pinned):
    table, po = pinned[0], pinned[1]
    nv = table.nv
    rng = np.random.default_rng(5)
    q, v, a = rng.uniform(-1.0, 1.0, (3, 5, nv))
    o = pinned[5]
    assert rel(jr.rnea(table, q, v, a), o.rnea(q, v, a).reshape(5, nv)) < 1e-11
    x = np.concatenate([q, v], 1)
    assert rel(jr.euler(table, x, 3 * a, po.dt[0]), o.integrate(x, 3 * a).reshape(5, 2 * nv)) < 1e-11
    jlog6 = orc.lib().orc_jlog6
    for frame in (len(table.frame_names) - 1, 1 + nv // 2):
        assert rel(jr.placement12(table, frame, q), o.frame_placement(frame, q)) < 1e-11
        # both Jacobian conventions through the checker's constraint Jacobians: FrameTranslation has the LOCAL_WORLD_ALIGNED
        # linear rows, FramePlacement has Jlog6(Mref^-1 M) x LOCAL Jacobian
        Mref = np.concatenate([rt.rpy(0.4, -0.3, 0.8).reshape(9), [0.2, -0.1, 0.3]])
        con = [_abi.ConstraintSpec(_abi.RES_FRAME_TRANSLATION, frame=frame, ref=np.zeros(3)),
               _abi.ConstraintSpec(_abi.RES_FRAME_PLACEMENT, frame=frame, ref=Mref)]
        oc = Oracle(table, _abi.PackedOcp(nv, TS, po.running, po.terminal, running_constraints=con), 1)
        for i in range(5):
            g, Gx, _ = oc.node_constraints(False, x[i], np.zeros(nv))
            lwa, loc = jr.frame_jacobian(table, frame, q[i]), jr.frame_jacobian(table, frame, q[i], local=True)
            assert rel(lwa[:3], Gx[:3, :nv]) < 1e-11
            R, p = jr.frame_placement(table, frame, q[i])
            Rr = Mref[:9].reshape(3, 3)
            rel12 = np.ascontiguousarray(np.concatenate([(Rr.T @ R).reshape(9), Rr.T @ (p - Mref[9:])]))
            J6 = np.empty((6, 6))
            jlog6(rel12.ctypes.data_as(C.c_void_p), J6.ctypes.data_as(C.c_void_p))
            assert rel(J6 @ loc, Gx[3:9, :nv]) < 1e-11
            assert rel(jr.residual(table, _abi.RES_FRAME_PLACEMENT, frame, 0, Mref, x[i], None), g[3:9]) < 1e-11


def test_helper_tiles_match_the_checker(pinned):
    table, want, got = pinned[0], pinned[6], pinned[7]
    assert got.shape == want.shape
    for field, s in _abi.tile_slices(table.nv).items():
        scale = max(np.abs(want[..., s]).max(), 1e-300)
        assert np.abs(got[..., s] - want[..., s]).max() <= 1e-10 * scale, field


def test_helper_lqr_matches_the_checker(pinned):
    """The tolerances of tests/test_hip_parity.py::test_direction_kernels_against_oracle."""
    table, o, tiles_o, tiles_h = pinned[0], pinned[5], pinned[6], pinned[7]
    Ko, ko, dxo, duo, kkto = o.direction(tiles_o)
    K, k, dx, du, kkt = jr.direction(table.nv, tiles_h)
    assert rel(dx, dxo) < 1e-9 and rel(du, duo) < 1e-9
    assert rel(K, Ko) < 1e-8
    np.testing.assert_allclose(kkt, kkto, rtol=1e-7)


def test_cartpole_closed_form():
    m_c, m_p, l, g = 1.3, 0.4, 0.7, 9.81
    t = jr.cartpole_table(m_c, m_p, l)
    rng = np.random.default_rng(1)
    q, qd, qdd = rng.uniform(-2.0, 2.0, (3, 20, 2))
    th, thd = q[:, 1], qd[:, 1]
    M = np.empty((20, 2, 2))
    M[:, 0, 0], M[:, 0, 1], M[:, 1, 0], M[:, 1, 1] = m_c + m_p, -m_p * l * np.cos(th), -m_p * l * np.cos(th), m_p * l * l
    nle = np.stack([m_p * l * np.sin(th) * thd ** 2, m_p * g * l * np.sin(th)], -1)
    want = (M @ qdd[..., None])[..., 0] + nle
    err = np.abs(jr.rnea(t, q, qd, qdd) - want).max()
    print("cart-pole closed form, max abs error", err)
    assert err < 1e-12
    assert np.abs(jr.crba(t, q) - M).max() < 1e-12


def test_gripper_at_rest_is_the_lumped_panda():
    """Lumping the fingers into link 7 is exact at the finger position the lumped table assumes (q = 0, at rest)."""
    g, p = rt.panda_gripper_table(), rt.panda_table()
    assert g.nv == 9 and list(g.joint_type) == [0] * 7 + [1, 1]
    rng = np.random.default_rng(2)
    q, qd, qdd = rng.uniform(-1.0, 1.0, (3, 10, 7))
    z = np.zeros((10, 2))
    cat = lambda a, b: np.concatenate([a, b], 1)  # noqa: E731
    want = jr.rnea(p, q, qd, qdd)
    got = jr.rnea(g, cat(q, z), cat(qd, z), cat(qdd, z))[:, :7]
    print("gripper at rest against the lumped table, relative", rel(got, want))
    assert rel(got, want) < 1e-12
    moved = jr.rnea(g, cat(q, z + 0.04), cat(qd, z + np.array([0.2, -0.1])), cat(qdd, z))[:, :7]
    print("fingers open and moving: arm torque change", np.abs(moved - want).max())
    assert np.abs(moved - want).max() > 1e-4
    # fingertips: at q = 0 both sit on the hand's tcp plane, and they open along the hand's +y / -y
    q0 = np.zeros(9)
    tcp = jr.frame_placement(g, g.frame_id("panda_hand_tcp"), q0)
    for name, sign in (("panda_leftfinger_tip", 1.0), ("panda_rightfinger_tip", -1.0)):
        f = g.frame_id(name)
        np.testing.assert_allclose(jr.frame_placement(g, f, q0)[1], tcp[1], atol=1e-14)
        q1 = q0.copy()
        q1[g.frame_parent[f]] = 0.04
        np.testing.assert_allclose(jr.frame_placement(g, f, q1)[1] - tcp[1], tcp[0] @ [0.0, 0.04 * sign, 0.0], atol=1e-14)


def test_host_layers_carry_the_joint_type():
    names = [f[0] for f in _abi.ModelDesc._fields_]
    assert names[:16] == ["nv", "nframes", "parent", "placement", "axis", "mass", "com", "inertia", "armature", "effort_limit", "gravity",
                          "frame_parent", "frame_placement", "frame_radius", "frame_halflen", "frame_box"]
    assert names[16:] == ["joint_type"]
    assert (rt.JOINT_REVOLUTE, rt.JOINT_PRISMATIC) == (0, 1)
    plain = _abi.PackedModel(rt.panda_table())
    assert rt.panda_table().joint_type is None and not plain.desc.joint_type  # NULL: all revolute
    g = rt.panda_gripper_table()
    pm = _abi.PackedModel(g)
    assert [pm.desc.joint_type[i] for i in range(9)] == [0] * 7 + [1, 1]
    assert pm.joint_type.dtype == np.int32
    assert list(g.with_armature(0.3).joint_type) == [0] * 7 + [1, 1] and np.all(g.with_armature(0.3).armature == 0.3)
    assert list(dataclasses.replace(g, name="x").joint_type) == [0] * 7 + [1, 1]
    assert list(g.with_geometry("s", 8, rt.se3(), radius=0.01).joint_type) == [0] * 7 + [1, 1]
    assert list(workloads.plant_tables(g, 2, seed=1)[1].joint_type) == [0] * 7 + [1, 1]
    from agimus_controller_amd.factory import robot_model

    rm = robot_model.panda_robot_models(gripper=True)
    assert rm.robot_model.nv == 9 and list(rm.table.joint_type) == [0] * 7 + [1, 1] and rm.q0.shape == (9,)
    assert robot_model.panda_robot_models().robot_model.nv == 7
    assert list(jr.with_prismatic(rt.chain_table(4), [2]).joint_type) == [0, 0, 1, 0]
