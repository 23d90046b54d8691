"""Clearance report on the device (agx_ocp_clearance / HipOcp.clearance / OCPCrocoGeneric.clearance, DESIGN.md section 4
"Diagnostics"): distances, witness points and the minimum of any pair list at the iterate or at given configurations.

References: the CPU checker (every pair, boxes included) and the numpy closed forms of tests/test_clearance.py (spheres and
capsules; pinned to the checker there), and for box pairs and degenerate capsule pairs the exact longdouble reference of
tests/test_clearance.py::degenerate_scene.  1e-12 absolute on distances throughout: the tolerance
tests/test_many_collision_costs.py uses for the distance of a pair row."""
import ctypes as C

import numpy as np
import pytest

import joint_ref as jr
import test_clearance as tc
from agimus_controller_amd import _abi, workloads
from agimus_controller_amd.factory import robot_tables as rt

pytestmark = pytest.mark.gpu

B = tc.B
TOL = 1e-12


def _handle(backend, table, T=2, batch=B):
    """A handle on a regulation problem (state and control rows only): none of the pairs is a row of it."""
    running, terminal = workloads.regulation_rows()
    return backend.HipOcp(table, _abi.PackedOcp(table.nv, [0.01] * T, list(running), list(terminal)), batch)


def _upload_q(h, q):
    """q [B][T + 1][nv] becomes the configuration part of the resident iterate (velocities and controls: seeded noise)."""
    rng = np.random.default_rng(9)
    xs = np.concatenate([q, rng.normal(size=q.shape)], -1)
    h.upload_warmstart(xs, rng.normal(size=(h.B, h.T, h.nv)))


_CHAIN64 = {}


def chain64(backend):
    """(table, pairs, q, checker dist, dist at the iterate, dist at q, witness at q) of the 64 pairs on the chain, T = 4: computed
    once, shared, left unchanged."""
    if not _CHAIN64:
        t, q, want = tc.chain_case()
        pairs = tc._pairs(64)
        h = _handle(backend, t, T=4)
        _upload_q(h, q)
        d_it = h.clearance(pairs)
        d_q, wit = h.clearance(pairs, q=q, witness=True)
        h.close()
        _CHAIN64["case"] = (t, pairs, q, want, d_it, d_q, wit)
    return _CHAIN64["case"]


def test_values_at_the_iterate_and_at_given_configurations(hip_backend):
    """64 pairs (four self pairs; link capsules against capsule, sphere and box obstacles), T = 4: the iterate after
    upload_warmstart and the same configurations as q agree with the checker on every pair and with the closed forms on every
    pair without a box to 1e-12, and with each other bitwise."""
    t, pairs, q, want, d_it, d_q, _ = chain64(hip_backend)
    assert d_it.shape == d_q.shape == (B, 5, 64)
    print("checker", np.abs(d_it - want).max())
    assert np.abs(d_it - want).max() <= TOL and np.abs(d_q - want).max() <= TOL
    closed = [k for k, (a, b) in enumerate(pairs) if not tc.is_box(t, t.frame_id(b))]
    ref = tc.reference(t, [pairs[k] for k in closed], q)
    print("closed forms", np.abs(d_it[..., closed] - ref).max())
    assert np.abs(d_it[..., closed] - ref).max() <= TOL
    assert np.array_equal(d_it, d_q)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 130])
def test_pair_counts_across_a_wave_and_a_workgroup_boundary(hip_backend, n):
    """n pairs, the list repeated to reach 130: every entry is bitwise its value in the 64-pair call, at the iterate and at q."""
    t, pairs, q, _, d64, _, wit64 = chain64(hip_backend)
    many = (pairs * 3)[:n]
    h = _handle(hip_backend, t, T=4)
    _upload_q(h, q)
    d_it = h.clearance(many)
    d_q, wit = h.clearance(many, q=q, witness=True)
    h.close()
    idx = np.arange(n) % 64
    assert d_it.shape == (B, 5, n)
    assert np.array_equal(d_it, d64[..., idx]) and np.array_equal(d_q, d64[..., idx])
    assert np.array_equal(wit, wit64[..., idx, :, :])


def test_witness_points_lie_on_the_surfaces(hip_backend):
    t, pairs, q, _, _, d, wit = chain64(hip_backend)
    assert wit.shape == (B, 5, 64, 3, 3)
    pa, pb, n = wit[..., 0, :], wit[..., 1, :], wit[..., 2, :]
    sep = d > 0.0
    assert sep.sum() > 0.9 * d.size
    gap = np.abs(pa - pb - d[..., None] * n).max(-1)
    norm = np.abs(np.sqrt((n * n).sum(-1)) - 1.0)
    print("pa - pb - d n", gap[sep].max(), "| |n| - 1 |", norm[sep].max())
    assert gap[sep].max() <= TOL and norm[sep].max() <= 1e-14
    for k, (a, b) in enumerate(pairs):
        sa = tc.surface_distance(t, t.frame_id(a), q, pa[..., k, :])
        sb = tc.surface_distance(t, t.frame_id(b), q, pb[..., k, :])
        s = sep[..., k]
        if s.any():
            assert sa[s].max() <= TOL and sb[s].max() <= TOL, (a, b, sa[s].max(), sb[s].max())


def test_overlapping_spheres_have_a_negative_distance(hip_backend):
    """The sphere obstacle ob1 moved into the sphere obstacle ob4 with set_geom_placement: centre distance minus the radii, and the
    witness relation holds with the normal pointing from b to a."""
    t = tc._chain()
    f1, f4 = t.frame_id("ob1"), t.frame_id("ob4")
    c4 = np.asarray(t.frame_placement, dtype=float).reshape(-1, 12)[f4, 9:]
    c1 = c4 + np.array([0.01, 0.02, -0.02])
    h = _handle(hip_backend, t)
    before = h.clearance([("ob1", "ob4")])
    h.set_geom_placement(f1, rt.se3(None, list(c1)))
    d, wit = h.clearance([("ob1", "ob4")], witness=True)
    h.close()
    want = 0.03 - (t.frame_radius[f1] + t.frame_radius[f4])
    assert want < 0.0 and np.all(before > 0.0)
    assert np.abs(d - want).max() <= TOL
    pa, pb, n = wit[..., 0, :], wit[..., 1, :], wit[..., 2, :]
    assert np.abs(pa - pb - d[..., None] * n).max() <= TOL
    np.testing.assert_allclose(n, np.broadcast_to((c1 - c4) / 0.03, n.shape), rtol=0, atol=1e-13)  # (c1 - c4 carries ulp(1) / 0.03)


def _with_links_and_obstacles(t, seed=17):
    """Capsules (r 0.03, half length 0.05) on joints 1 .. 8 and six seeded world spheres."""
    for j in range(1, 9):
        t = t.with_geometry(f"cap{j}", j, rt.se3(None, [0.0, 0.0, 0.04]), 0.03, 0.05)
    rng = np.random.default_rng(seed)
    for i in range(6):
        d = rng.normal(size=3)
        t = t.with_geometry(f"ob{i}", -1, rt.se3(None, list(rng.uniform(0.3, 0.9) * d / np.linalg.norm(d))), rng.uniform(0.03, 0.07))
    return t


def _self_pairs(t):
    """(pairs of joints 1 .. 8 of which one is an ancestor of the other, pairs on two branches)."""
    def ancestors(i):
        out = set()
        while t.parent[i] >= 0:
            i = int(t.parent[i])
            out.add(i)
        return out

    one, two = [], []
    for a in range(1, 9):
        for b in range(a + 2, 9):  # (not a link against its own parent link)
            (one if a in ancestors(b) else two).append((f"cap{a}", f"cap{b}"))
    return one, two


SIZES = {"tree9_padded_to_16": lambda: rt.tree_table(9, seed=3), "tree16": lambda: rt.tree_table(16, seed=3),
         "tree20_at_30": lambda: rt.tree_table(20, seed=3), "chain31_at_32": lambda: rt.chain_table(31, seed=3)}


@pytest.mark.parametrize("size", list(SIZES))
def test_model_sizes(hip_backend, size):
    """One case per capacity above 7 joints: 20 pairs with self pairs on one and on two branches, m = 5 random configurations,
    1e-12 against the closed forms."""
    t = _with_links_and_obstacles(SIZES[size]())
    one, two = _self_pairs(t)
    assert one and (two or size.startswith("chain"))
    self_pairs = one[:2] + two[:2]
    world = [(f"cap{j}", f"ob{i}") for i in range(6) for j in range(1, 9)]
    pairs = (self_pairs + world)[:20]
    q = np.random.default_rng(21).uniform(-1.0, 1.0, (B, 5, t.nv))
    h = _handle(hip_backend, t)
    d = h.clearance(pairs, q=q)
    h.close()
    want = tc.reference(t, pairs, q)
    print(size, np.abs(d - want).max())
    assert d.shape == (B, 5, 20) and np.abs(d - want).max() <= TOL


def _sphere_links(t, joints):
    for j in joints:
        t = t.with_geometry(f"s{j}", j, rt.se3(None, [0.02, -0.01, 0.03]), radius=0.02)
    return t


@pytest.mark.parametrize("model", ["tree9_prismatic", "panda_gripper"])
def test_prismatic_joints(hip_backend, model):
    if model == "tree9_prismatic":
        t = _sphere_links(jr.with_prismatic(rt.tree_table(9, seed=3), [0, 4, 7]), range(9))
    else:
        t = _sphere_links(rt.panda_gripper_table(), range(9))
    names = [f"s{j}" for j in range(9)]
    pairs = [(a, b) for i, a in enumerate(names) for b in names[i + 1:]]
    q = np.random.default_rng(4).uniform(-0.6, 0.6, (B, 3, t.nv))
    h = _handle(hip_backend, t)
    d = h.clearance(pairs, q=q)
    _upload_q(h, q)
    d_it = h.clearance(pairs)
    h.close()
    want = tc.reference(t, pairs, q)
    print(model, np.abs(d - want).max())
    assert np.abs(d - want).max() <= TOL and np.array_equal(d, d_it)


def test_every_instance_sees_its_own_world(hip_backend):
    """Panda collision table with three more obstacles, set_obstacle_placements: instance b equals a handle whose model has the
    obstacles at b's placements; after clear_obstacle_placements every instance is back on the model's."""
    table = rt.panda_collision_table(0.1, obstacle_xyz=(0.45, 0.1, 0.45), obstacle_radius=0.08, obstacle_length=0.3,
                                     obstacles=workloads.random_obstacles(3))
    frames = ["obstacle", "ob1", "ob2"]  # ob0 keeps the model's placement
    pairs = [(c, o) for o in ("obstacle", "ob0", "ob1", "ob2") for c in workloads.PANDA_LINK_CAPSULES] + workloads.PANDA_SELF_COLLISION_PAIRS
    se3 = workloads.obstacle_placements(table, frames, B, 5)
    q = np.random.default_rng(8).uniform(-1.0, 1.0, (B, 3, 7))
    h = _handle(hip_backend, table)
    _upload_q(h, q)
    nominal = h.clearance(pairs)
    h.set_obstacle_placements(frames, se3)
    got, got_q = h.clearance(pairs), h.clearance(pairs, q=q)
    assert np.array_equal(got, got_q)
    assert np.abs(got[0] - nominal[0]).max() <= TOL and np.abs(got[1:] - nominal[1:]).max() > 1e-3
    for b, tb in enumerate(workloads.world_tables(table, frames, se3)):
        hb = _handle(hip_backend, tb, batch=1)
        want = hb.clearance(pairs, q=q[b:b + 1])
        hb.close()
        assert np.abs(got[b] - want[0]).max() <= TOL, b
    h.clear_obstacle_placements()
    assert np.array_equal(h.clearance(pairs), nominal)
    h.close()


def test_minimum_is_the_first_argmin(hip_backend):
    """min_dist / min_where against numpy's min and first argmin over dist of the same call; pairs listed twice make ties."""
    t, pairs, q, *_ = chain64(hip_backend)
    many = pairs[60:] + pairs + pairs  # 132 pairs, every one of them at least twice: the minimum of every instance is a tie
    h = _handle(hip_backend, t, T=4)
    _upload_q(h, q)
    for kw in ({}, {"q": np.concatenate([q, q[:, ::-1], q], 1)}):  # 5 samples: one chunk; 15: two chunks, the minimum in several
        d, (dmin, where) = h.clearance(many, minimum=True, **kw)
        flat = d.reshape(B, -1)
        first = flat.argmin(1)
        assert np.array_equal(dmin, flat.min(1))
        assert np.array_equal(where[:, 0], first // len(many)) and np.array_equal(where[:, 1], first % len(many))
        assert all((flat[b] == dmin[b]).sum() >= 2 for b in range(B))
    h.close()


def _panda_loop(backend, probe, n_steps=4, T=8):
    """A resident sine MPC loop on the Panda with link capsules; probe(h) runs between the steps."""
    table = rt.panda_collision_table(0.1, obstacle_xyz=(0.45, 0.1, 0.45), obstacle_radius=0.08, obstacle_length=0.3)
    tcp = table.frame_id("panda_hand_tcp")
    running, terminal = workloads.goal_reaching_rows(tcp)
    po = _abi.PackedOcp(7, [0.01] * T, running, terminal, termination_tolerance=1e-3, max_qp_iters=100)
    h = backend.HipOcp(table, po, B)
    q0, amp, puls, scale, t0 = workloads.sine_batch_params(B, nv=7, lower=table.lower_position_limit, upper=table.upper_position_limit)
    w = workloads.SINE_WEIGHTS
    h.sine_trajectory(n_steps + T + 4, 0.01, q0, amp, puls, scale, t0, w["w_q"], w["w_qdot"], w["w_effort"], w["w_pose"], tcp)
    out = []
    for k in range(n_steps):
        if k > 0 and probe is not None:
            probe(h)
        h.mpc_step(k, 10, first=(k == 0))
        first = h.download_first(copy=True)
        out.append(h.download() + tuple(first[:3]))
    counts = (h.carry_counts(), h.first_pack_counts())
    h.close()
    return out, counts


def test_the_call_only_reads(hip_backend):
    """solve, clearance, the same solve again: the bits of two solves without the call.  A resident sine MPC loop of four steps
    with the call between the steps: the same results, carry_counts and first_pack_counts as the loop without it."""
    table = rt.panda_collision_table(0.1, obstacle_xyz=(0.45, 0.1, 0.45), obstacle_radius=0.08, obstacle_length=0.3)
    tcp = table.frame_id("panda_hand_tcp")
    rows = workloads.collision_avoidance_rows(table, tcp, alpha=0.05)
    po, ref, x0, xs, us = workloads.random_goal_problem(table, 8, 0.01, B, 23, frame=tcp, rows=rows)
    pairs = [(c, "obstacle") for c in workloads.PANDA_LINK_CAPSULES] + workloads.PANDA_SELF_COLLISION_PAIRS
    q = np.random.default_rng(2).uniform(-1.0, 1.0, (B, 11, 7))

    def probe(h):
        h.clearance(pairs)
        h.clearance(pairs, q=q, witness=True, minimum=True)

    runs = []
    for with_call in (False, True):
        h = hip_backend.HipOcp(table, po, B)
        h.set_refs(ref)
        a = h.solve(x0, xs, us, 6)
        if with_call:
            probe(h)
        runs.append((a, h.solve(x0, xs, us, 6)))
        h.close()
    for r0, r1 in zip(*runs):  # first solves, second solves
        for v0, v1 in zip(r0, r1):
            assert v0.tobytes() == v1.tobytes()
    plain, counts_plain = _panda_loop(hip_backend, None)
    probed, counts_probed = _panda_loop(hip_backend, probe)
    assert counts_plain == counts_probed and counts_plain[0][0] >= 1, (counts_plain, counts_probed)
    for k, (r0, r1) in enumerate(zip(plain, probed)):
        for v0, v1 in zip(r0, r1):
            assert v0.tobytes() == v1.tobytes(), k


def test_refusals_name_the_call_and_leave_the_handle_usable(hip_backend):
    t = tc._chain()
    h = _handle(hip_backend, t, T=4)
    L = hip_backend.lib()
    f = t.frame_id
    out = np.empty((B, 5, 2))

    def call(handle, n, fa, fb, q, m, dist=out):
        p = lambda a: None if a is None else np.ascontiguousarray(a).ctypes.data_as(C.c_void_p)  # noqa: E731
        fa = None if fa is None else np.asarray(fa, dtype=np.int32)
        fb = None if fb is None else np.asarray(fb, dtype=np.int32)
        rc = L.agx_ocp_clearance(handle, C.c_int(n), p(fa), p(fb), p(q), C.c_int(m), p(dist), None, None, None)
        return rc, L.agx_last_error().decode()

    good = ([f("cap1"), f("cap2")], [f("cap3"), f("ob0")])
    q5 = np.zeros((B, 5, 6))
    cases = [
        (call(None, 2, *good, None, 5), "agx_ocp_clearance"),
        (call(h._h, 2, None, good[1], None, 5), "null pair arrays"),
        (call(h._h, 2, good[0], None, None, 5), "null pair arrays"),
        (call(h._h, 0, *good, None, 5), "n_pairs"),
        (call(h._h, 2, *good, q5, 0), "m must be at least 1"),
        (call(h._h, 2, *good, None, 4), "T + 1 = 5"),
        (call(h._h, 2, [f("cap1"), len(t.frame_names)], good[1], None, 5), "pair 1: frame %d out of range" % len(t.frame_names)),
        (call(h._h, 2, good[0], [f("cap3"), -1], None, 5), "pair 1: frame -1 out of range"),
        (call(h._h, 2, [f("tool"), f("cap2")], good[1], None, 5), "pair 0: frame %d carries no collision geometry" % f("tool")),
        (call(h._h, 2, [f("cap1"), f("ob2")], [f("cap3"), f("ob5")], None, 5), "pair 1: box / box collision pairs are not supported"),
    ]
    for (rc, msg), word in cases:
        assert rc != 0 and msg.startswith("agx_ocp_clearance") and word in msg, (rc, msg, word)
    with pytest.raises(hip_backend.HipError, match="pair 0: box / box collision pairs are not supported"):
        h.clearance([("ob2", "ob5")])
    d = h.clearance([("cap1", "cap3"), ("cap2", "ob0")], q=q5)
    assert d.shape == (B, 5, 2) and np.abs(d - tc.reference(t, [("cap1", "cap3"), ("cap2", "ob0")], q5)).max() <= TOL
    h.close()


def test_class_surface(hip_backend):
    """OCPCrocoGeneric from ocp_traj_tracking_collision_avoidance.yaml on a collision model with more pairs than the YAML uses."""
    from agimus_controller_amd import se3
    from agimus_controller_amd.factory.robot_model import RobotModelParameters, RobotModels
    from agimus_controller_amd.ocp.ocp_croco_generic import OCPCrocoGeneric
    from agimus_controller_amd.ocp_param_base import DTFactorsNSeq, OCPParamsBaseCroco
    from agimus_controller_amd.trajectory import TrajectoryPoint, TrajectoryPointWeights, WeightedTrajectoryPoint
    from agimus_controller_amd.workloads import PANDA_Q0

    T, dt = 10, 0.02
    table = rt.panda_collision_table(0.1, obstacle_xyz=(0.42, 0.05, 0.55), obstacle_radius=0.06, obstacle_length=0.2)
    model_pairs = [("panda_link7_capsule_0", "obstacle")] + [(c, "obstacle") for c in workloads.PANDA_LINK_CAPSULES[:4]] + \
        workloads.PANDA_SELF_COLLISION_PAIRS
    rm = RobotModels(RobotModelParameters(table=table, armature=table.armature, q0=PANDA_Q0, collision_pairs=model_pairs))
    params = OCPParamsBaseCroco(dt=dt, horizon_size=T, dt_factor_n_seq=DTFactorsNSeq(factors=[1], n_steps=[T]), solver_iters=10, qp_iters=100,
                                callbacks=False)
    ocp = OCPCrocoGeneric(rm, params, OCPCrocoGeneric.get_default_yaml_file("ocp_traj_tracking_collision_avoidance.yaml"))
    start = ocp._hip.frame_placement(table.frame_id("panda_hand_tcp"), PANDA_Q0)[0]
    goal = se3.SE3(start[:9].reshape(3, 3), start[9:] + np.array([0.12, 0.05, 0.05]))
    pt = WeightedTrajectoryPoint(
        TrajectoryPoint(robot_configuration=PANDA_Q0, robot_velocity=np.zeros(7), robot_effort=np.zeros(7), end_effector_poses={"panda_hand_tcp": goal}),
        TrajectoryPointWeights(w_robot_configuration=0.01 * np.ones(7), w_robot_velocity=0.1 * np.ones(7), w_robot_effort=1e-4 * np.ones(7),
                               w_end_effector_poses={"panda_hand_tcp": 50.0 * np.ones(6)}, w_collision_avoidance=2.0))
    ocp.set_reference_weighted_trajectory([pt] * (T + 1))
    x0 = np.concatenate([PANDA_Q0, np.zeros(7)])
    ocp.solve(x0, [x0] * (T + 1), [np.zeros(7)] * T)
    names, d = ocp.clearance()
    assert names == [f"{a}|{b}" for a, b in model_pairs] and d.shape == (T + 1, len(model_pairs))
    own = ocp._hip.clearance([model_pairs[0]])
    assert np.array_equal(d[:, 0], own[0, :, 0])
    states = np.array(ocp.ocp_results.states)
    names_s, d_s, wit = ocp.clearance(states, witness=True)
    assert names_s == names and np.array_equal(d_s, d) and wit.shape == (T + 1, len(model_pairs), 3, 3)
    assert np.array_equal(ocp.clearance(states[:, :7])[1], d)
    assert np.abs(d - tc.reference(table, model_pairs, states[:, :7])).max() <= TOL
    with pytest.raises(ValueError, match="states"):
        ocp.clearance(states[:, :5])



def test_box_and_degenerate_capsule_pairs_against_the_exact_reference(hip_backend):
    """The 60 pairs of tc.degenerate_scene (box against capsule and sphere: generic, parallel to a face, parallel to an edge,
    vertex, end point, sphere centre inside; capsules parallel, tilted by 1e-3 / 1e-6 / 1e-8 rad, collinear, crossing, against a
    sphere), each as (a, b) and (b, a), through clearance(q=..., witness=True): distance to 1e-12 of the longdouble value; where
    the pair is separated pa - pb = d n, |n| = 1 and both witness points lie on their surfaces.  With crossing axes and with the
    sphere centre inside the box only the distance is asserted (the normal is not defined)."""
    t, cases = tc.degenerate_scene()
    pairs = [(a, b) for a, b, _, _ in cases]
    want = np.array([w for _, _, w, _ in cases])
    q = np.zeros((B, 2, t.nv))
    h = _handle(hip_backend, t)
    d, wit = h.clearance(pairs, q=q, witness=True)
    h.close()
    assert d.shape == (B, 2, len(pairs))
    err = np.abs(d - want).max((0, 1))
    for (a, b), e, w in zip(pairs, err, want):
        print(f"{a} / {b}: exact {w:.17g} err {e:.2e}")
    assert err.max() <= TOL, [(p, e) for p, e in zip(pairs, err) if e > TOL]
    pa, pb, n = wit[..., 0, :], wit[..., 1, :], wit[..., 2, :]
    for k, (a, b, w, witness) in enumerate(cases):
        if not witness:
            continue
        assert w > 0.0
        gap = np.abs(pa[..., k, :] - pb[..., k, :] - d[..., k, None] * n[..., k, :]).max()
        norm = np.abs(np.sqrt((n[..., k, :] ** 2).sum(-1)) - 1.0).max()
        sa = tc.surface_distance(t, t.frame_id(a), q, pa[..., k, :]).max()
        sb = tc.surface_distance(t, t.frame_id(b), q, pb[..., k, :]).max()
        print(f"{a} / {b}: pa - pb - d n {gap:.2e} | |n| - 1 | {norm:.2e} surfaces {sa:.2e} {sb:.2e}")
        assert gap <= TOL and norm <= 1e-14 and sa <= TOL and sb <= TOL, (a, b, gap, norm, sa, sb)
