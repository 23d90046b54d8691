"""Forward pass, node KKT pass and head of the step in one launch per instance (k_step_tail; default on)
against the three launches it replaces (HipOcp.set_step_tail(False)).  Loads, stores and where the shares travel differ; no
operand, product or summation order does, so everything a solve leaves behind must be bitwise equal: xs, us, K, the direction
(dx, du), the node shares and every status word, after a cold solve and after three resident MPC steps.  The switch is a setter
on the handle: both handles live in this process.  AGX_MX2_SEGMENTS=0 in every case, so that the small batches of a test
take the one-wave sweeps the kernel sits behind.  One case pins the default to the checker with the tolerances of
tests/test_node_passes_gpu.py::test_default_against_the_checker.  Every comparison also asks the two handles how many k_step_tail
launches they made: the default one some, the other none -- otherwise both would have run the three launches and agreed for nothing."""

import os

import numpy as np
import pytest

import launch_paths as lp
from agimus_controller_amd import _abi, workloads
from agimus_controller_amd.factory import robot_tables as rt

pytestmark = pytest.mark.gpu

DT = 0.01
N_STEPS = 4  # the cold solve and three resident MPC steps


def _handle(backend, tail, table, po, B, extra=None):
    env = {"AGX_MX2_SEGMENTS": "0", **(extra or {})}
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        h = backend.HipOcp(table, po, B)
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    if not tail:
        h.set_step_tail(False)  # (a fresh handle has it on)
    return h


def _left_behind(h):
    xs, us, K, st = h.download()
    dx, du, ns = h.last_direction()
    return dict(xs=xs, us=us, K=K, dx=dx, du=du, nodestat=ns, st=np.array(st), tail_launches=h.step_tail_launches())


def _run_sine(backend, tail, table, po, B, frame, max_iters, extra=None):
    """The cold solve (first MPC step) and three more steps on the resident sine trajectory."""
    h = _handle(backend, tail, table, po, B, extra)
    nv = table.nv
    q0, amp, puls, scale, t0 = workloads.sine_batch_params(B, nv=nv, seed0=1234, q0=(None if nv == 7 else np.zeros(nv)),
                                                           lower=table.lower_position_limit, upper=table.upper_position_limit)
    w = workloads.SINE_WEIGHTS
    h.sine_trajectory(N_STEPS + po.horizon + 4, DT, q0, amp, puls, scale, t0, w["w_q"], w["w_qdot"], w["w_effort"], w["w_pose"], frame)
    out = []
    for k in range(N_STEPS):
        h.mpc_step(k, max_iters[k], first=1 if k == 0 else 0)
        out.append(_left_behind(h))
    h.close()
    return out


def _run_refs(backend, tail, table, po, ref, x0, xs, us, iters, extra=None):
    """The cold solve from the caller's warm start, then three steps of the resident loop: shift, x0 from the prediction, solve."""
    B = x0.shape[0]
    h = _handle(backend, tail, table, po, B, extra)
    h.set_refs(ref)
    h.upload_x0(x0)
    h.upload_warmstart(xs, us)
    out = []
    for k in range(N_STEPS):
        if k:
            h.x0_from_prediction()
            h.shift_warmstart()
        h.solve_resident(iters)
        out.append(_left_behind(h))
    h.close()
    return out


def _assert_bitwise(fused, three):
    assert len(fused) == len(three) == N_STEPS
    # the paths really differ: one k_step_tail launch per SQP iteration of a step on the default handle, none on the other
    assert fused[0]["tail_launches"] >= 1 and all(b["tail_launches"] > a["tail_launches"] for a, b in zip(fused, fused[1:])), \
        [r["tail_launches"] for r in fused]
    assert all(r["tail_launches"] == 0 for r in three), [r["tail_launches"] for r in three]
    for k, (rf, rt3) in enumerate(zip(fused, three)):
        for field in rf["st"].dtype.names:
            assert np.array_equal(rf["st"][field], rt3["st"][field], equal_nan=True), f"step {k}: status word {field} differs"
        for name in ("xs", "us", "K", "dx", "du", "nodestat"):
            a, b = rf[name], rt3[name]
            assert a.tobytes() == b.tobytes(), f"step {k}: {name} differs in {int(np.sum(a != b))} places (NaNs compared as bits)"
    return fused


def _sine_case(backend, table, po, B, frame, max_iters=(10,) * N_STEPS, extra=None):
    return _assert_bitwise(_run_sine(backend, True, table, po, B, frame, max_iters, extra),
                           _run_sine(backend, False, table, po, B, frame, max_iters, extra))


def _refs_case(backend, table, po, ref, x0, xs, us, iters, extra=None):
    return _assert_bitwise(_run_refs(backend, True, table, po, ref, x0, xs, us, iters, extra),
                           _run_refs(backend, False, table, po, ref, x0, xs, us, iters, extra))


def _panda(T):
    table = rt.panda_table(0.1)
    tcp = table.frame_id("panda_hand_tcp")
    running, terminal = workloads.goal_reaching_rows(tcp)
    return table, tcp, _abi.PackedOcp(7, [DT] * T, running, terminal, termination_tolerance=1e-3, max_qp_iters=100)


@pytest.mark.parametrize("B,T", [(3, 1), (3, 7), (2, 9)], ids=["one_running_node", "below_the_prefetch_depth", "two_groups_and_a_remainder"])
def test_short_horizons(hip_backend, B, T):
    """T = 1: one running node and the terminal one.  T = 7: every node of the forward pass goes through the one-at-a-time loop
    in front of the pipelined one, and the eight nodes fill one group of the node pass.  T = 9: a second group of two nodes, one
    remainder node in front of one pipelined group."""
    table, tcp, po = _panda(T)
    _sine_case(hip_backend, table, po, B, tcp)


def test_mixed_step_lengths(hip_backend):
    """B = 5, T = 23, dt 0.01 / 0.02 / 0.04 along the horizon (three node groups, seven remainder nodes)."""
    table = rt.panda_table(0.1)
    po, ref, x0, xs, us = workloads.random_goal_problem(table, 23, DT, 5, 6, frame=table.frame_id("panda_hand_tcp"),
                                                        timesteps=[0.01] * 12 + [0.02] * 7 + [0.04] * 4)
    _refs_case(hip_backend, table, po, ref, x0, xs, us, 12)


def test_five_joints_padded_to_seven(hip_backend):
    """A 5-joint chain in the 7-joint capacity: the lanes l8 >= nv and the padded rows of the lane grid."""
    table = rt.chain_table(5, seed=25)
    frame = len(table.frame_names) - 1
    running, terminal = workloads.goal_reaching_rows(frame)
    po = _abi.PackedOcp(5, [DT] * 9, running, terminal, termination_tolerance=1e-3, max_qp_iters=100)
    _sine_case(hip_backend, table, po, 5, frame)


def test_workgroups_of_finished_instances(hip_backend):
    """B = 40, T = 7, max_iter = 1 on every second step (the case of tests/test_node_passes_gpu.py): where instances of one step
    finish after different numbers of iterations, the workgroups of the finished ones leave at once next to workgroups that work."""
    table, tcp, po = _panda(7)
    runs = _sine_case(hip_backend, table, po, 40, tcp, max_iters=(10, 1, 10, 1))
    assert any(len(np.unique(r["st"]["iter"])) > 1 for r in runs), "no step with finished instances next to working ones"


def test_large_batch_hand_off(hip_backend):
    """The counters of a batch above 204 reach the host through k_publish3, not through the last workgroup of the kernel, and a
    record packed by a converging workgroup is not fenced at system scope: the same small case under AGX_FOLD_PUBLISH=0."""
    table, tcp, po = _panda(9)
    _sine_case(hip_backend, table, po, 11, tcp, extra={"AGX_FOLD_PUBLISH": "0"})


def test_line_search_rejects_the_full_step(hip_backend):
    """`goal` of tests/launch_paths.py (B = 9, T = 13, mixed dt; seed chosen there on the CPU): the checker rejects alpha = 1 in an
    instance, so the head hands a trial on that the first round refuses, and the instances finish in different iterations."""
    p = lp.problem("goal")
    runs = _refs_case(hip_backend, p.table, p.po, p.ref, p.x0, p.xs, p.us, p.iters)
    assert np.any(runs[0]["st"]["flags"] & 4), "no step length was rejected: the case does not reach the second round"
    assert len(set(runs[0]["st"]["iter"])) >= 2


def test_iteration_cap_of_one(hip_backend):
    """max_iter = 1: the gains sweep runs between the head and the search, nothing is paired, the fix-up on exit serves the rest."""
    p = lp.problem("goal")
    _refs_case(hip_backend, p.table, p.po, p.ref, p.x0, p.xs, p.us, 1)


def _obstacle_entering_problem():
    """Two instances of the collision workload of bench.py without its distance constraint, T = 200, on sine references built
    as the resident generator builds them: the reference of the first one (instance 14 of the benchmark batch) ends inside the
    obstacle, the second one (instance 0) is a regular instance."""
    import bench
    from oracle.oracle import Oracle

    T, sel = 200, [14, 0]
    table, tcp, po = bench.make_problem(T, "collision")
    po = _abi.PackedOcp(7, [DT] * T, po.running, po.terminal, termination_tolerance=1e-3, max_qp_iters=100)
    q0, amp, puls, scale, t0 = (a[sel] for a in workloads.sine_batch_params(16, nv=7, seed0=1234, lower=table.lower_position_limit,
                                                                            upper=table.upper_position_limit))
    B = len(sel)
    o = Oracle(table, po, B)
    w = workloads.SINE_WEIGHTS
    ref = po.new_ref_tile(B)
    xs, us = np.empty((B, T + 1, 14)), np.empty((B, T, 7))
    for t in range(T + 1):
        tt = t0 + t * DT
        s_ = np.clip(tt[:, None] / scale, 0.0, 1.0)
        inside = (s_ > 0) & (s_ < 1)
        ramp = 10 * s_**3 - 15 * s_**4 + 6 * s_**5
        dramp = np.where(inside, (30 * s_**2 - 60 * s_**3 + 30 * s_**4) / scale, 0.0)
        ddramp = np.where(inside, (60 * s_ - 180 * s_**2 + 120 * s_**3) / scale**2, 0.0)
        sw, cw = np.sin(puls * tt[:, None]), np.cos(puls * tt[:, None])
        q = q0 + amp * ramp * sw
        dq = amp * (dramp * sw + ramp * puls * cw)
        ddq = amp * (ddramp * sw + 2 * dramp * puls * cw - ramp * puls**2 * sw)
        u, pose = o.rnea(q, dq, ddq).reshape(B, 7), o.frame_placement(tcp, q)
        xs[:, t] = np.concatenate([q, dq], 1)
        if t < T:
            us[:, t] = u
        rows, offs = (po.terminal, po.terminal_offsets) if t == T else (po.running, po.running_offsets)
        for r, off in zip(rows, offs):
            seg = ref[:, t, off:]
            seg[:, 0] = 1.0
            if r.kind == _abi.RES_STATE:
                seg[:, 1:15], seg[:, 15:22], seg[:, 22:29] = xs[:, t], w["w_q"], w["w_qdot"]
            elif r.kind == _abi.RES_CONTROL:
                seg[:, 1:8], seg[:, 8:15] = u, w["w_effort"]
            elif r.kind == _abi.RES_FRAME_PLACEMENT:
                seg[:, 1:13], seg[:, 13:19] = pose, w["w_pose"]
            else:
                seg[:, 1] = 0.0
    return table, po, ref, xs[:, 0].copy(), xs, us


def test_discarded_direction(hip_backend):
    """The obstacle-entering pair above (T = 200: the nodes beyond the LDS window
    too): the QuadExp collision cost has negative curvature near the obstacle, the sweep of instance 0 meets a non-positive
    pivot (dir_fail), the head discards the direction -- NaN KKT, flags 7, iterate unchanged (the checker: flags [7, 0], checked on
    the CPU) -- while instance 1 converges."""
    table, po, ref, x0, xs, us = _obstacle_entering_problem()
    runs = _refs_case(hip_backend, table, po, ref, x0, xs, us, 4)
    st = runs[0]["st"]
    assert st["flags"][0] == 7 and np.isnan(st["kkt"][0]) and np.array_equal(runs[0]["xs"][0], xs[0])
    assert st["flags"][1] == 0 and st["solved"][1] == 1


def test_default_against_the_checker(hip_backend, panda, monkeypatch):
    """The default alone against the oracle: direction kernels at a fixed point and a full solve (tolerances as in
    tests/test_node_passes_gpu.py::test_default_against_the_checker)."""
    from oracle.oracle import Oracle

    monkeypatch.setenv("AGX_MX2_SEGMENTS", "0")
    rel = lambda a, b: float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))  # noqa: E731
    tcp = panda.frame_id("panda_hand_tcp")
    B, T = 3, 13
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
