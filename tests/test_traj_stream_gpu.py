"""Streamed resident trajectory on the device (agx_traj_stream_*): a ring of samples with a mirrored tail that
the caller appends to and releases from while MPC steps run on it.

The yardstick is the one-shot resident trajectory on the same samples (`generic_trajectory_weighted`): k_traj_append and
k_sine_fill share the per-sample device function, the window of a streamed handle is the same pointer arithmetic on the slot
k0 mod capacity, so EVERYTHING a step hands out must be bitwise equal -- at every step, across the wrap of the ring, with
uniform and non-uniform horizons, with and without the tile carry, for padded models and wide cost sets.

Shapes: the smallest at which wrap, mirror and chunk boundaries all occur (T = 5: windows of 6 in a ring of 8, of 10 in a ring of
12; T = 4 in a ring of 7).  The feeder releases the past before each step and appends only when the next window needs it, in
chunks of 6, 1, 3, 5, 2, 4, ... samples cut to the room the ring has: a window of 6 in a ring of 8 leaves room for at most 3
once the loop runs, so after the first two chunks the sizes are 3, 3, 2, 3, ... at moving slot offsets; `_feed` returns the
log and the tests assert that a chunk crossed the wrap and wrote mirror and plain slots."""

import numpy as np
import pytest

from agimus_controller_amd import _abi, workloads
from agimus_controller_amd.factory import robot_tables as rt
from agimus_controller_amd.ocp_param_base import DTFactorsNSeq
from agimus_controller_amd.se3 import SE3
from agimus_controller_amd.trajectory import TrajectoryPoint, TrajectoryPointWeights, WeightedTrajectoryPoint
from agimus_controller_amd.trajectory_stream import DeviceTrajectoryBuffer, StreamedMPC

pytestmark = pytest.mark.gpu

DT = 0.01
MAX_ITER = 4
CHUNKS = (6, 1, 3, 5, 2, 4)


class Problem:
    """Model, cost rows and N samples per instance with pose and pose-weight schedules (and optionally a collision-weight one)."""

    def __init__(self, backend, table, frame, running, terminal, B, T, N, q0, seed, w_collision=False):
        nv = table.nv
        self.backend, self.table, self.frame, self.B, self.T, self.N, self.nv = backend, table, frame, B, T, N, nv
        self.po = _abi.PackedOcp(nv, [DT] * T, running, terminal, termination_tolerance=1e-3, max_qp_iters=100)
        rng = np.random.default_rng(seed)
        q0 = np.asarray(q0, dtype=float) + rng.normal(0.0, 0.02, (B, nv))
        self.q, self.dq, self.ddq = workloads.generic_batch_arrays(B, N, DT, nv=nv, seed0=seed, q0=q0)
        self.w_q, self.w_qdot, self.w_effort = rng.uniform(0.5, 1.5, nv), rng.uniform(0.05, 0.2, nv), rng.uniform(1e-4, 1e-3, nv)
        k = np.arange(N)[None, :, None]
        b = np.arange(B)[:, None, None]
        self.w_pose = np.array([2.0, 2.0, 2.0, 0.5, 0.5, 0.5]) * (1.0 + 0.5 * np.sin(0.3 * k + b + np.arange(6)))
        h = backend.HipOcp(table, self.po, 1)
        self.pose = h.frame_placement(frame, self.q.reshape(-1, nv)).reshape(B, N, 12)  # the sample's own pose, moved by a schedule
        h.close()
        self.pose[..., 9:] += 0.01 * np.sin(0.2 * k + b + np.arange(3))
        self.w_coll = rng.uniform(0.05, 0.2, (B, N)) if w_collision else None
        self._ref = {}

    def handle(self):
        return self.backend.HipOcp(self.table, self.po, self.B)

    def one_shot(self, idx=None, n_points=None):
        """The one-shot resident trajectory over the first n_points samples (default: all N)."""
        h = self.handle()
        s = slice(0, n_points or self.N)
        h.generic_trajectory_weighted(self.q[:, s], self.dq[:, s], self.ddq[:, s], self.w_q, self.w_qdot, self.w_effort, self.w_pose[:, s], self.frame,
                                      pose=self.pose[:, s], w_collision=None if self.w_coll is None else self.w_coll[:, s])
        if idx is not None:
            h.set_horizon_indexes(idx)
        return h

    def streamed(self, capacity, max_span, idx=None):
        h = self.handle()
        h.stream_trajectory(capacity, max_span, self.w_q, self.w_qdot, self.w_effort, np.zeros(6), self.frame)
        if idx is not None:
            h.set_horizon_indexes(idx)
        assert h.stream_range() == (0, 0)
        return h

    def append(self, h, lo, hi):
        s = slice(lo, hi)
        h.stream_append(self.q[:, s], self.dq[:, s], self.ddq[:, s], pose=self.pose[:, s], w_pose=self.w_pose[:, s],
                        w_collision=None if self.w_coll is None else self.w_coll[:, s])

    def reference_run(self, n_steps, idx=None):
        """The loop of the one-shot handle over n_steps + span points (first = 1, then first = 0), computed once per
        (n_steps, idx) and shared; never modified."""
        key = (n_steps, None if idx is None else tuple(idx))
        if key not in self._ref:
            h = self.one_shot(idx, n_points=n_steps + 1 + (self.T if idx is None else idx[-1]))
            out = []
            for k in range(n_steps):
                h.mpc_step(k, MAX_ITER, first=1 if k == 0 else 0)
                out.append(_snapshot(h))
            for r in out:
                assert all(np.all(np.isfinite(a)) for a in r[:3])
            assert not np.array_equal(out[0][0], out[-1][0])  # the loop moves
            self._ref[key] = (h, out)
        return self._ref[key]


def _snapshot(h):
    xs, us, K, st = h.download()
    return xs, us, K, np.array(st)


def _assert_same(got, want, what):
    for name, a, b in zip(("xs", "us", "K"), got[:3], want[:3]):
        assert np.array_equal(a, b), f"{what}: {name} differs (max |diff| {np.abs(a - b).max():.3e})"
    for field in want[3].dtype.names:
        assert np.array_equal(got[3][field], want[3][field], equal_nan=True), f"{what}: status field {field} differs"


def _feed(pr, h, k, span, capacity, log, state, n_total):
    """Before step k: release the past, then append chunks until the window [k, k + span) is there."""
    first, end = h.stream_range()
    if k > first:
        h.stream_release(k)
        first = k
    while end < k + span:
        room = capacity - (end - first)
        m = min(CHUNKS[state["chunk"] % len(CHUNKS)], room, n_total - end)
        assert m >= 1
        state["chunk"] += 1
        pr.append(h, end, end + m)
        log.append((end, m))
        end += m
    assert h.stream_range() == (first, end)


def _streamed_run(pr, n_steps, capacity, span, idx=None, h=None):
    h = h or pr.streamed(capacity, span, idx)
    log, state, out = [], {"chunk": 0}, []
    for k in range(n_steps):
        _feed(pr, h, k, span, capacity, log, state, n_steps + span)  # the points the one-shot handle holds
        h.mpc_step(k, MAX_ITER, first=1 if k == 0 else 0)
        out.append(_snapshot(h))
    return h, out, log


def _assert_feed_covers_wrap_and_mirror(log, capacity, span):
    """A chunk crossed the wrap, and a chunk wrote slots with and without a mirror."""
    crossed = mixed = False
    for lo, m in log:
        slots = [_abi.ring_slots(k, capacity, span) for k in range(lo, lo + m)]
        crossed |= any(slots[i + 1][0] < slots[i][0] for i in range(m - 1))
        mixed |= any(s[1] is None for s in slots) and any(s[1] is not None for s in slots)
    assert crossed and mixed, log


def _assert_points_and_tiles(pr, hs, ha, capacity, span):
    """traj_point / traj_tile of retained logical samples, one in a mirror-covered slot and one outside, against the one-shot handle."""
    first, end = hs.stream_range()
    with_mirror = [k for k in range(first, end) if _abi.ring_slots(k, capacity, span)[1] is not None]
    without = [k for k in range(first, end) if _abi.ring_slots(k, capacity, span)[1] is None]
    assert with_mirror and without
    for k in (with_mirror[0], without[0], end - 1):
        for a, b in zip(hs.traj_point(k), ha.traj_point(k)):
            assert np.array_equal(a, b), k
        for terminal in (False, True):
            assert np.array_equal(hs.traj_tile(k, terminal), ha.traj_tile(k, terminal)), (k, terminal)


def _compare_with_one_shot(pr, n_steps, capacity, span, idx=None):
    ha, want = pr.reference_run(n_steps, idx)
    hs, got, log = _streamed_run(pr, n_steps, capacity, span, idx)
    assert n_steps >= 2 * capacity, "the window start must wrap at least twice"
    for k, (g, w) in enumerate(zip(got, want)):
        _assert_same(g, w, f"step {k}")
    _assert_feed_covers_wrap_and_mirror(log, capacity, span)
    _assert_points_and_tiles(pr, hs, ha, capacity, span)
    hs.close()


@pytest.fixture(scope="module")
def panda(hip_backend):
    table = rt.panda_table(0.1)
    tcp = table.frame_id("panda_hand_tcp")
    running, terminal = workloads.goal_reaching_rows(tcp)
    pr = Problem(hip_backend, table, tcp, running, terminal, B=3, T=5, N=40, q0=workloads.PANDA_Q0, seed=500)
    yield pr
    for h, _ in pr._ref.values():
        h.close()


# 1 ---------------------------------------------------------------------------------------------------------------------------
def test_streamed_loop_is_bitwise_the_one_shot_loop(panda):
    """Panda, B = 3, T = 5, N = 24 + 6 = 30 points: ring of 8 for windows of 6, 24 steps (the window start wraps three times)."""
    _compare_with_one_shot(panda, 24, capacity=8, span=6)


# 2 ---------------------------------------------------------------------------------------------------------------------------
def test_non_uniform_horizon(panda):
    """idx = [0,1,2,4,6,9]: windows of 10 samples in a ring of 12, gathered by k_gather_window from the slot k0 mod 12; 30 steps."""
    _compare_with_one_shot(panda, 30, capacity=12, span=10, idx=[0, 1, 2, 4, 6, 9])


# 3 ---------------------------------------------------------------------------------------------------------------------------
def test_tile_carry_goes_on_across_the_wrap(panda, monkeypatch):
    """The streamed loop twice in fresh handles, AGX_TILE_CARRY = 0 and 1: bitwise equal over 20 steps (test 1 compares the default,
    carrying, loop with the one-shot handle).  tests/test_tile_carry_gpu.py observes nothing but that equality, so that the
    second run really carries is read from the in-situ profile, switched on in both runs: its counter of derivative passes over
    all B T running nodes does not count the first pass of a carrying step (tile carry, launch shape), every other
    pass is the same in both runs, so the two counters differ by the 19 steps that follow a step."""
    n_steps = 20
    runs, full_passes = [], []
    for carry in ("0", "1"):
        monkeypatch.setenv("AGX_TILE_CARRY", carry)
        h = panda.streamed(8, 6)
        h.profile(True)
        _, out, _ = _streamed_run(panda, n_steps, 8, 6, h=h)
        full_passes.append(h.profile(False)[1][0])
        h.close()
        runs.append(out)
    for k, (off, on) in enumerate(zip(*runs)):
        _assert_same(on, off, f"step {k}, carry on against off")
    print("passes over all running nodes, carry off / on:", full_passes)
    assert full_passes[0] - full_passes[1] == n_steps - 1, full_passes


# 4 ---------------------------------------------------------------------------------------------------------------------------
def _gripper_problem(backend):
    table = rt.panda_gripper_table(0.1)
    tcp = table.frame_id("panda_hand_tcp")
    running, terminal = workloads.goal_reaching_rows(tcp)
    q0 = np.concatenate([workloads.PANDA_Q0, [0.02, 0.02]])
    return Problem(backend, table, tcp, running, terminal, B=3, T=4, N=24, q0=q0, seed=600)


def _chain7_problem(backend):
    """chain_table(7) with a capsule on joints 2 .. 6 and four world spheres: 3 + 12 cost rows, a wide cost set."""
    t = rt.chain_table(7, seed=3)
    for j in range(2, 7):
        t = t.with_geometry(f"cap{j}", j, rt.se3(None, [0.0, 0.0, 0.05]), 0.04, 0.06)
    rng = np.random.default_rng(5)
    for i in range(4):
        d = rng.normal(size=3)
        t = t.with_geometry(f"ob{i}", -1, rt.se3(None, list(rng.uniform(0.6, 0.9) * d / np.linalg.norm(d))), rng.uniform(0.03, 0.07), 0.0)
    tool = t.frame_id("tool")
    running, terminal = workloads.goal_reaching_rows(tool)
    pairs = [(f"cap{j}", f"ob{i}") for i in range(4) for j in (2, 4, 6)]
    pc = workloads.collision_pair_costs(t, pairs, _abi.ACT_QUAD_EXP, 0.05, 0.1)
    assert len(running) + len(pc) == 15
    return Problem(backend, t, tool, list(running) + pc, list(terminal) + pc, B=3, T=4, N=24, q0=np.zeros(7), seed=700, w_collision=True)


@pytest.mark.parametrize("which", ["panda_gripper", "chain7_wide"])
def test_model_sizes_and_wide_cost_sets(hip_backend, which):
    """The Panda with its real gripper (nv = 9 at the capacity of 16: pad joints in the staged chunk) and a 7-joint chain with
    3 + 12 cost rows and a per-sample collision weight (k_cost_pairs_fill_ring); T = 4, ring of 7, 16 steps."""
    pr = _gripper_problem(hip_backend) if which == "panda_gripper" else _chain7_problem(hip_backend)
    if which == "chain7_wide":
        h = pr.handle()
        assert h.cost_wide
        h.close()
    _compare_with_one_shot(pr, 16, capacity=7, span=5)
    if pr.w_coll is not None:  # the scheduled weight is in the pair rows of the streamed tiles (and differs from the YAML weight)
        hs = pr.streamed(7, 5)
        pr.append(hs, 0, 5)
        tile = hs.traj_tile(3)
        for p in range(12):
            o = pr.po.running_offsets[3 + p]
            assert np.array_equal(tile[:, o], pr.w_coll[:, 3]) and np.all(tile[:, o + 1] == 1.0)
        hs.close()
    for h, _ in pr._ref.values():
        h.close()


# 5 ---------------------------------------------------------------------------------------------------------------------------
def test_ordering_between_the_copy_stream_and_the_solver(panda):
    """No host synchronisation between an append and the step that reads it, and none between a step and the append that
    overwrites the slots it read: the events order the two streams."""
    pr, C, span = panda, 12, 6
    want = pr.reference_run(24)[1]
    h = pr.streamed(C, span)
    assert h.stream_joins() == (0, 0)
    h.stream_timing(True)  # events around every join (solver stream) and every appended piece (copy stream)
    pr.append(h, 0, 6)
    assert h.stream_joins() == (0, 1)  # enqueued on the copy stream, nobody has been made to wait for it yet
    h.mpc_step(0, MAX_ITER, first=1)
    assert h.stream_joins() == (1, 0)  # the step made the solver stream wait for the append's event
    # five samples and at once a window whose last sample is one of them
    pr.append(h, 6, 11)
    assert h.stream_joins() == (1, 1)
    h.mpc_step(1, MAX_ITER, first=0)
    assert h.stream_joins() == (2, 0)
    _assert_same(_snapshot(h), want[1], "step 1, right behind the append of samples 6 .. 10")
    for k in range(2, 5):
        h.mpc_step(k, MAX_ITER, first=0)
    assert h.stream_joins() == (2, 0)  # windows inside what was joined: no further waits
    pr.append(h, 11, 12)  # the ring is full: samples 0 .. 11 in slots 0 .. 11
    assert h.stream_range() == (0, 12)
    h.mpc_step(5, MAX_ITER, first=0)  # window [5, 11)
    assert h.stream_joins() == (2, 1)  # sample 11 is outside that window: its append stays pending
    # the step has returned: release what it read up to sample 5 and overwrite slots 0 .. 5 at once
    h.stream_release(6)
    pr.append(h, 12, 18)
    assert h.stream_joins() == (2, 2)
    got = _snapshot(h)
    _assert_same(got, want[5], "step 5, downloaded after its slots were overwritten")
    h.mpc_step(6, MAX_ITER, first=0)  # window [6, 12) reaches sample 11, not yet 12
    assert h.stream_joins() == (3, 1)
    _assert_same(_snapshot(h), want[6], "step 6")
    h.mpc_step(7, MAX_ITER, first=0)  # window [7, 13): through the mirror, and into the append of 12 .. 17
    assert h.stream_joins() == (4, 0)
    _assert_same(_snapshot(h), want[7], "step 7")
    # the device work of the last append once more (time_kernel(10)): the handle and the loop are as they were
    assert h.time_kernel(10, 3) > 0.0
    assert h.stream_range() == (6, 18) and h.stream_joins() == (4, 0)
    ms, count = h.stream_timing(False)
    assert count == [4, 4] and ms[0] >= 0.0 and ms[1] > 0.0, (ms, count)  # four joins, four appended pieces
    assert h.stream_timing(False)[1] == [0, 0]  # switching off cleared the sums
    for k in range(8, 10):  # windows [8, 14), [9, 15)
        h.mpc_step(k, MAX_ITER, first=0)
        _assert_same(_snapshot(h), want[k], f"step {k}")
    h.close()


# 6 ---------------------------------------------------------------------------------------------------------------------------
def test_refusals_change_nothing(panda, hip_backend):
    pr = panda
    want = pr.reference_run(24)[1]
    Err = hip_backend.HipError
    h = pr.streamed(8, 6)
    pr.append(h, 0, 6)
    h.mpc_step(0, MAX_ITER, first=1)
    h.stream_release(1)
    rng_before = h.stream_range()
    assert rng_before == (1, 6)
    q, dq, ddq = pr.q, pr.dq, pr.ddq
    weights = (pr.w_q, pr.w_qdot, pr.w_effort, np.zeros(6), pr.frame)

    def refused(match, fn):
        with pytest.raises(Err, match=match):
            fn()
        assert h.stream_range() == rng_before

    refused(r"overflow the ring, release the past first \(first 1, end 6, capacity 8\)", lambda: pr.append(h, 6, 10))
    refused(r"agx_traj_set_window: samples \[1, 7\) are not inside the retained range \[first, end\) = \[1, 6\)",
            lambda: h.mpc_step(1, MAX_ITER, first=0))
    refused(r"agx_traj_set_window: samples \[0, 6\) are not inside the retained range \[first, end\) = \[1, 6\)", lambda: h.set_window(0))
    refused(r"agx_traj_get_point: samples \[0, 1\) are not inside", lambda: h.traj_point(0))
    refused(r"agx_traj_stream_release: 7 is outside \[first, end\] = \[1, 6\]", lambda: h.stream_release(7))
    refused(r"agx_traj_stream_release: 0 is outside", lambda: h.stream_release(0))
    refused("m must be at least 1", lambda: h.stream_append(q[:, :0], dq[:, :0], ddq[:, :0]))
    bad = q[:, 6:7].copy()
    bad[1, 0, 3] = np.nan
    refused("non-finite value in q", lambda: h.stream_append(bad, dq[:, 6:7], ddq[:, 6:7]))
    refused(r"max_span 5 is below the T \+ 1 = 6 samples of a window", lambda: h.stream_trajectory(8, 5, *weights))
    refused("capacity 5 is below max_span 6", lambda: h.stream_trajectory(5, 6, *weights))
    refused("frame id out of range", lambda: h.stream_trajectory(8, 6, *weights[:4], 10_000))
    refused(r"idx\[T\] \+ 1 = 10 samples, the streamed trajectory was created with max_span 6", lambda: h.set_horizon_indexes([0, 1, 2, 4, 6, 9]))
    # the refused calls left the loop (and the tile carry) as it was: the next step is the one-shot loop's
    pr.append(h, 6, 7)
    h.mpc_step(1, MAX_ITER, first=0)
    _assert_same(_snapshot(h), want[1], "step 1 after the refusals")
    h.close()
    # a handle with a one-shot trajectory has no stream
    ha = pr.one_shot()
    ha.mpc_step(0, MAX_ITER, first=1)
    for fn in (lambda: pr.append(ha, 0, 1), lambda: ha.stream_release(0), ha.stream_range):
        with pytest.raises(Err, match="the handle has no streamed trajectory"):
            fn()
    ha.mpc_step(1, MAX_ITER, first=0)
    _assert_same(_snapshot(ha), want[1], "one-shot handle, step 1 after the refusal")
    with pytest.raises(Err, match="which = 10 needs a streamed trajectory with an append"):
        ha.time_kernel(10, 1)
    # horizon indexes set BEFORE the ring is created count too: a window of 10 does not fit a mirror made for 6
    ha.set_horizon_indexes([0, 1, 2, 4, 6, 9])
    with pytest.raises(Err, match=r"agx_traj_stream_create: the horizon indexes of the handle cover idx\[T\] \+ 1 = 10 samples, max_span is 6"):
        ha.stream_trajectory(12, 6, *weights)
    with pytest.raises(Err, match="the handle has no streamed trajectory"):  # the refused create left the one-shot trajectory
        ha.stream_range()
    ha.set_horizon_indexes(None)
    ha.mpc_step(0, MAX_ITER, first=1)
    _assert_same(_snapshot(ha), want[0], "one-shot handle after the refused stream create")
    # ... and a streamed handle that gets a one-shot trajectory stops being one
    ha.stream_trajectory(8, 6, *weights)
    assert ha.stream_range() == (0, 0)
    with pytest.raises(Err, match="which = 10 needs a streamed trajectory with an append"):
        ha.time_kernel(10, 1)
    with pytest.raises(Err, match=r"are not inside the retained range \[first, end\) = \[0, 0\)"):
        ha.mpc_step(0, MAX_ITER, first=1)
    ha.generic_trajectory_weighted(pr.q, pr.dq, pr.ddq, pr.w_q, pr.w_qdot, pr.w_effort, pr.w_pose, pr.frame, pose=pr.pose)
    with pytest.raises(Err, match="the handle has no streamed trajectory"):
        ha.stream_range()
    ha.mpc_step(0, MAX_ITER, first=1)
    _assert_same(_snapshot(ha), want[0], "one-shot trajectory created over a streamed one")
    ha.close()


# 7 ---------------------------------------------------------------------------------------------------------------------------
def test_streamed_mpc_against_a_one_shot_handle_driven_by_hand(hip_backend):
    """B = 1, Panda, the rows of ocp_goal_reaching.yaml; points arrive one at a time between runs, 20 solved runs over a ring of
    2 (T + 1) samples.  By hand: the same points as a one-shot weighted trajectory, upload_x0 + mpc_step(first = 1, then 2)."""
    table = rt.panda_table(0.1)
    tcp = table.frame_id("panda_hand_tcp")
    running, terminal = workloads.goal_reaching_rows(tcp)
    T, n_runs = 6, 20
    N = T + n_runs
    pr = Problem(hip_backend, table, tcp, running, terminal, B=1, T=T, N=N, q0=workloads.PANDA_Q0, seed=800)
    points = []
    for k in range(N):
        p = pr.pose[0, k]
        pt = TrajectoryPoint(id=100 + k, time_ns=k, robot_configuration=pr.q[0, k], robot_velocity=pr.dq[0, k], robot_acceleration=pr.ddq[0, k],
                             end_effector_poses={"panda_hand_tcp": SE3(p[:9].reshape(3, 3), p[9:])})
        w = TrajectoryPointWeights(w_robot_configuration=pr.w_q, w_robot_velocity=pr.w_qdot, w_robot_acceleration=np.zeros(7),
                                   w_robot_effort=pr.w_effort, w_end_effector_poses={"panda_hand_tcp": pr.w_pose[0, k]})
        points.append(WeightedTrajectoryPoint(pt, w))
    noise = np.random.default_rng(9).normal(0.0, 1e-3, (n_runs, 14))

    hs = pr.handle()
    buf = DeviceTrajectoryBuffer(hs, DTFactorsNSeq(factors=[1], n_steps=[T]), 2 * (T + 1), "panda_hand_tcp", pr.w_q, pr.w_qdot, pr.w_effort)
    mpc = StreamedMPC()
    mpc.setup(hs, buf, MAX_ITER)
    ha = pr.one_shot()
    x_meas = np.concatenate([pr.q[0, 0], pr.dq[0, 0]])
    solved = 0
    for r in range(N):
        mpc.append_trajectory_point(points[r])
        state = TrajectoryPoint(robot_configuration=x_meas[:7], robot_velocity=x_meas[7:])
        res = mpc.run(state, 0)
        if r < T:
            assert res is None and len(buf) == r + 1
            continue
        s = r - T
        ha.upload_x0(x_meas[None])
        ha.mpc_step(s, MAX_ITER, first=1 if s == 0 else 2)
        us0, K0, x1, st = ha.download_first()
        assert np.array_equal(res.feed_forward_terms[0], us0[0]) and np.array_equal(res.ricatti_gains[0], K0[0])
        assert np.array_equal(res.states[1], x1[0]) and np.array_equal(res.states[0], ha.download_x0()[0])
        dbg = mpc.mpc_debug_data
        assert dbg.reference_id == 100 + s and dbg.ocp.nb_iter == st["iter"][0] and dbg.ocp.kkt_norm == st["kkt"][0]
        assert hs.stream_range() == (s + 1, r + 1) and len(buf) == T
        x_meas = x1[0] + noise[s]
        solved += 1
    assert solved == n_runs
    hs.close()
    ha.close()
