"""Lifetime of what a handle allocates (csrc/agx_host_handle.hpp: DeviceOwner): nothing survives agx_ocp_destroy, a failed
trajectory build leaves nothing behind, and the buffers that swap roles (agx_ocp_set_refs_async) are still freed once each.

Shapes: the Panda with goal rows at B = 3, T = 6; the constrained `con` problem (B = 4, T = 12) and the 9-joint `nv9` problem
(second capacity group) of launch_paths.py.  Memory is the free memory of the device as the HIP runtime reports it (free_bytes).

Measured on the MI355X in one call, five cycles after one warm-up cycle: the parent commit (its library loaded through AGX_LIB)
lost 0 bytes, this code lost 0 bytes.  The parent returns to the byte, so the bar for the cycles is 0.  The failed build may
keep one allocation granule of the runtime (2 MiB): each of its three arrays takes more than that, so one that stays shows."""
import ctypes as C

import numpy as np
import pytest

import launch_paths as lp
from agimus_controller_amd import workloads
from agimus_controller_amd.factory import robot_tables as rt

pytestmark = pytest.mark.gpu

B, T, DT, ITERS = 3, 6, 0.01, 4
N_CYCLES = 5
N_SMALL = 600  # cycles of test_no_small_block_survives_destroy: more small blocks than a chunk of the runtime holds (512)
GRANULE = 2 << 20  # the runtime takes device memory in 2 MiB granules
PARENT_LOSS = 0    # bytes the parent commit lost over N_CYCLES cycles (module docstring): it returns to the byte, and so must this code


def free_bytes(backend):
    """Free memory of the device as the HIP runtime the library runs on reports it (hipMemGetInfo, what torch.cuda.mem_get_info
    wraps).  Asked of that runtime directly: the runtime torch bundles does not find the device once another one holds it."""
    backend.lib()
    path = next(line.split()[-1] for line in open("/proc/self/maps") if "libamdhip64" in line)
    hip = C.CDLL(path)  # (the copy that is already mapped)
    free, total = C.c_size_t(0), C.c_size_t(0)
    assert hip.hipDeviceSynchronize() == 0 and hip.hipMemGetInfo(C.byref(free), C.byref(total)) == 0
    return int(free.value)


class Goal:
    """Panda (with the world-fixed obstacle geometry, so that a placement table can be set), goal rows, B = 3, T = 6."""

    def __init__(self):
        self.table = rt.panda_collision_table(0.1, obstacle_xyz=(0.45, 0.1, 0.45), obstacle_radius=0.08, obstacle_length=0.3)
        self.tcp = self.table.frame_id("panda_hand_tcp")
        self.po, self.ref, self.x0, self.xs, self.us = workloads.random_goal_problem(self.table, T, DT, B, 17, frame=self.tcp)
        self.frames = self.po.default_frames(B)
        self.frames[:, ::2, 2] = self.table.frame_id("panda_link5")  # the running placement row of every other node looks at another frame
        self.sine = workloads.sine_batch_params(B, lower=self.table.lower_position_limit, upper=self.table.upper_position_limit)
        self.w = workloads.SINE_WEIGHTS
        self.samples = workloads.generic_batch_arrays(B, T + 6, DT)
        self.inertials = workloads.stack_inertials(workloads.plant_tables(self.table, B, seed=5))
        self.obstacles = (["obstacle"], workloads.obstacle_placements(self.table, ["obstacle"], B, 0, 0.1, 0.5))

    def pinned(self, backend):
        """Page-locked staging tile and result arrays, allocated once (they are the caller's, not the handle's)."""
        if not hasattr(self, "_pinned"):
            staged = backend.pinned_array(self.ref.shape)
            staged[...] = self.ref
            nv = self.table.nv
            self._pinned = (staged, [backend.pinned_array(s) for s in ((B, T + 1, 2 * nv), (B, T, nv), (B, T, nv, 2 * nv))])
        return self._pinned

    def sine_trajectory(self, h, n_points):
        w = self.w
        h.sine_trajectory(n_points, DT, *self.sine, w["w_q"], w["w_qdot"], w["w_effort"], w["w_pose"], self.tcp)


@pytest.fixture(scope="module")
def goal():
    return Goal()


def cycle(backend, g, light=False):
    """Creates handles, touches every lazily allocated resource once, destroys them.  light: the 7-joint handle alone, and of the
    solves and MPC steps, which allocate nothing after the first solve, only that one with a single iteration."""
    iters = 1 if light else ITERS
    h = backend.HipOcp(g.table, g.po, B)
    w = g.w
    h.set_refs(g.ref)
    h.profile(True)  # event pairs around the launches of the SQP loop
    h.solve(g.x0, g.xs, g.us, iters)
    h.profile(False)
    staged, out = g.pinned(backend)
    h.set_refs_async(staged, g.frames)  # copy stream, its events, the back tile and the back frame table
    h.refs_activate()
    light or h.solve_resident(iters)
    h.download_async(*out)  # the snapshot
    h.download_wait()
    h.download_first()  # the first-node block
    h.iter_log(4)
    light or h.solve_resident(iters)
    h.read_iter_log()
    h.item_costs()
    h.set_model_inertials(*g.inertials)
    h.set_plant_inertials(*g.inertials)
    h.set_obstacle_placements(*g.obstacles)
    h.integrate(g.x0, g.us[:, 0])  # the scratch block
    h.calc_diff()  # the canonical tiles
    h.set_horizon_indexes([0, 1, 2, 3, 4, 6, 8])
    g.sine_trajectory(h, T + 8)
    light or h.mpc_step(0, iters, True)
    h.set_horizon_indexes(None)
    h.generic_trajectory(*g.samples, w["w_q"], w["w_qdot"], w["w_effort"], w["w_pose"], g.tcp)
    light or h.mpc_step(0, iters, True)
    h.stream_trajectory(T + 2, T + 1, w["w_q"], w["w_qdot"], w["w_effort"], w["w_pose"], g.tcp)
    h.stream_timing(True)  # event pairs on both streams
    h.stream_append(*(a[:, :T + 1] for a in g.samples))
    h.set_window(0) if light else h.mpc_step(0, iters, True)  # (the window joins the append: timing events on the solver stream)
    h.stream_timing(False)
    h.close()
    for name in () if light else ("con", "nv9"):  # the ADMM buffers and the LQR gains next to them; the second capacity group and its sigma tiles
        p = lp.problem(name)
        h = backend.HipOcp(p.table, p.po, p.B)
        p.prepare(h)
        h.profile(True)
        h.solve(p.x0, p.xs, p.us, 2)
        h.download_first()
        h.iter_log(2)
        h.item_costs()
        h.close()


def lost_over_cycles(backend, g, n=N_CYCLES):
    cycle(backend, g)  # warm-up: code objects, the runtime's own pools
    before = free_bytes(backend)
    for _ in range(n):
        cycle(backend, g)
    return before - free_bytes(backend)


def test_nothing_survives_destroy(hip_backend, goal):
    lost = lost_over_cycles(hip_backend, goal)
    print(f"device memory lost over {N_CYCLES} create / use / destroy cycles: {lost} bytes (parent commit: {PARENT_LOSS})")
    assert lost <= PARENT_LOSS


def test_no_small_block_survives_destroy(hip_backend, goal):
    """Most buffers of these shapes are far below a granule, and one that stays does not move the free memory of the device.  But the
    runtime carves small blocks out of 2 MiB chunks at 4 KiB each (measured: 20 000 blocks of 28 B and of 4 096 B both take
    83 886 080 B: 512 to a chunk), so N_SMALL = 600 blocks that stay do not fit the chunk they start in and another one is taken.
    One small block left per cycle is therefore seen as a loss of a granule or more -- often far more, since a chunk goes back to
    the device only when it is empty.  Measured: a build of this library that did not free the horizon index table lost
    1 218 445 312 B over these 600 cycles (and 2 MiB after 100 bare create / set_horizon_indexes / destroy cycles, 4 MiB after
    500, 6 MiB after 1 000); the parent's library and this one lose 0 bytes.  About 6 s: 600 handles at 3.7 ms to create."""
    cycle(hip_backend, goal, light=True)
    before = free_bytes(hip_backend)
    for _ in range(N_SMALL):
        cycle(hip_backend, goal, light=True)
    lost = before - free_bytes(hip_backend)
    print(f"device memory lost over {N_SMALL} cycles of the 7-joint handle: {lost} bytes")
    assert lost <= PARENT_LOSS


def test_a_failed_build_leaves_nothing(hip_backend, goal):
    """The failing call of test_sin_wave_cartesian_space_gpu.py (the target of instance 2 is out of reach), on a handle that has a
    trajectory and on enough points that each array takes more than a granule: the old trajectory and the half-built one both go."""
    g, w = goal, goal.w
    n = 4000
    q0, amp, puls = workloads.cartesian_sine_batch_params(B, lower=g.table.lower_position_limit, upper=g.table.upper_position_limit)
    far = amp.copy()
    far[2] = [5.0, 0.0, 0.0]
    h = hip_backend.HipOcp(g.table, g.po, B)
    before = free_bytes(hip_backend)
    h.generic_trajectory(*workloads.generic_batch_arrays(B, n, DT), w["w_q"], w["w_qdot"], w["w_effort"], w["w_pose"], g.tcp)
    taken = before - free_bytes(hip_backend)
    print(f"device memory a resident trajectory of {n} samples takes: {taken} bytes")
    assert taken >= 8 * B * n * 2 * h.stride  # the probe sees d_traj alone: what the failing build below drops, and its own arrays, would show
    with pytest.raises(hip_backend.HipError, match="inverse kinematics failed to converge: instance 2"):
        h.cartesian_sine_trajectory(n, DT, q0, far, puls, w["w_q"], w["w_qdot"], w["w_effort"], w["w_pose"], g.tcp, it_max=50)
    held = before - free_bytes(hip_backend)
    print(f"device memory the failed build still holds: {held} bytes")
    assert held <= GRANULE
    with pytest.raises(hip_backend.HipError, match="agx_traj_set_window: no resident trajectory"):
        h.set_window(0)
    with pytest.raises(hip_backend.HipError, match="no resident trajectory"):
        h.traj_point(0)
    fresh = hip_backend.HipOcp(g.table, g.po, B)
    results = []
    for handle in (h, fresh):
        g.sine_trajectory(handle, T + 8)
        handle.mpc_step(0, ITERS, True)
        handle.mpc_step(1, ITERS, False)
        results.append(handle.download())
        handle.close()
    for got, want in zip(*results):
        assert np.array_equal(np.asarray(got), np.asarray(want))


def test_swapped_buffers(hip_backend, goal):
    """Tile and frame table staged by set_refs_async swap roles with the handle's own at every activation; both fields are still the
    handle's to free, whichever block they hold."""
    g = goal
    h = hip_backend.HipOcp(g.table, g.po, B)
    h.set_refs(g.ref, g.frames)
    xs_want = h.solve(g.x0, g.xs, g.us, ITERS)[0]
    h.close()
    plain = hip_backend.HipOcp(g.table, g.po, B)
    plain.set_refs(g.ref)
    assert not np.array_equal(plain.solve(g.x0, g.xs, g.us, ITERS)[0], xs_want)  # the frame table matters
    plain.close()
    staged, staged_frames = hip_backend.pinned_array(g.ref.shape), hip_backend.pinned_array(g.frames.shape, np.int32)
    staged[...] = g.ref
    staged_frames[...] = g.frames
    h = hip_backend.HipOcp(g.table, g.po, B)
    for _ in range(2):
        h.set_refs_async(staged, staged_frames)
        h.refs_activate()
        assert np.array_equal(h.solve(g.x0, g.xs, g.us, ITERS)[0], xs_want)
    h.close()
