"""The reference's streaming loop on the device-resident path.

Upstream the planner `append`s points to an unbounded `TrajectoryBuffer` while `MPC.run` pops one per step with `clear_past`
(trajectory.py:181-231, mpc.py:30-41).  `DeviceTrajectoryBuffer` has that surface and keeps the samples in the handle's streamed
ring (`HipOcp.stream_trajectory` / `stream_append` / `stream_release`): what travels per step is the new points, not the
[B][T+1][stride] tile, and the window moves by pointer arithmetic with the tile carry intact.  `StreamedMPC` has the surface of
`MPC` on top of it.  `mpc.py`, `trajectory.py` and `OCPCrocoGeneric` (the host path) are untouched."""

from __future__ import annotations

import time

import numpy as np

from .mpc_data import MPCDebugData, OCPDebugData, OCPResults
from .ocp_param_base import DTFactorsNSeq
from .se3 import as_se3_12
from .trajectory import TrajectoryBuffer, TrajectoryPoint, WeightedTrajectoryPoint


def _vec(w, n) -> np.ndarray:
    """Scalar or vector weights -> n-vector (size-1 arrays broadcast like the ROS publisher's), as OCPCrocoGeneric reads them."""
    a = np.asarray(w, dtype=np.float64).reshape(-1)
    if a.size == 1:
        return np.full(n, a[0])
    assert a.size == n, f"expected {n} weights, got {a.size}"
    return a.copy()


class DeviceTrajectoryBuffer:
    """`TrajectoryBuffer` whose points live in the streamed ring of a `HipOcp`.

    `hip`       the handle (B instances); the buffer creates its ring;
    `capacity`  samples the ring retains per instance (at least `horizon_indexes[-1] + 1`);
    `frame`     key of the end-effector pose and pose weights in the points (`end_effector_poses[frame]`,
                `w_end_effector_poses[frame]`); the frame rows look at `frame_id` (default: the table's frame of that name);
    `w_q`, `w_qdot`, `w_effort`  joint weights: the ring holds them per handle, like the other resident generators, so a
                point whose `w_robot_configuration` / `w_robot_velocity` / `w_robot_effort` differ is refused.

    For B = 1 an item is a `WeightedTrajectoryPoint`, for B > 1 a sequence of B of them (one per instance).  Points wait on the
    host until `flush()` (called by `clear_past`, by `StreamedMPC.run`, and by hand) sends all that fit in one `stream_append`;
    those that do not fit yet stay pending, so the buffer is unbounded like the reference's.  Per sample the device takes
    q, dq, ddq (a missing acceleration counts as zero) and computes the effort by inverse dynamics, as every resident generator
    does; the pose, the pose weights and `w_collision_avoidance` are the point's."""

    def __init__(self, hip, dt_factor_n_seq: DTFactorsNSeq, capacity: int, frame: str, w_q, w_qdot, w_effort, frame_id: int | None = None):
        self._hip = hip
        self.B, self.nv = int(hip.B), int(hip.nv)
        self.dt_factor_n_seq = dt_factor_n_seq
        self.horizon_indexes = TrajectoryBuffer(dt_factor_n_seq).horizon_indexes
        assert len(self.horizon_indexes) == hip.T + 1, f"the horizon indexes give {len(self.horizon_indexes) - 1} nodes, the handle has T = {hip.T}"
        self.capacity = int(capacity)
        self.frame = frame
        self.frame_id = hip.table.frame_id(frame) if frame_id is None else int(frame_id)
        self.w_q, self.w_qdot, self.w_effort = _vec(w_q, self.nv), _vec(w_qdot, self.nv), _vec(w_effort, self.nv)
        self._pending: list = []  # items not sent yet
        self._ids: list = []  # id of instance 0's point, for every retained or pending sample
        self._first = self._end = 0  # the ring's retained logical range [first, end)
        hip.stream_trajectory(self.capacity, self.max_span, self.w_q, self.w_qdot, self.w_effort, np.zeros(6), self.frame_id)
        hip.set_horizon_indexes(self.horizon_indexes)

    @property
    def max_span(self) -> int:
        """Samples a window covers."""
        return self.horizon_indexes[-1] + 1

    @property
    def first(self) -> int:
        """Logical index of the oldest retained sample: the window start of the next MPC step."""
        return self._first

    @property
    def retained(self) -> int:
        """Samples on the device (without the pending ones)."""
        return self._end - self._first

    # -- TrajectoryBuffer surface ---------------------------------------------
    def append(self, item):
        pts = self._as_instance_points(item)
        for b, wp in enumerate(pts):
            self._check_joint_weights(wp, b)
        self._pending.append(pts)
        self._ids.append(pts[0].point.id)

    def extend(self, items):
        for item in items:
            self.append(item)

    def clear_past(self):
        """Drops the oldest sample (TrajectoryBuffer.clear_past): `stream_release(first + 1)`."""
        if len(self) == 0:
            return
        if self.retained == 0:
            self.flush()
        self._hip.stream_release(self._first + 1)
        self._first += 1
        del self._ids[0]

    def __len__(self):
        return self.retained + len(self._pending)

    def reference_id(self, i: int = 0):
        """`point.id` of instance 0's i-th sample counted from the oldest retained one."""
        return self._ids[i]

    # -- device side ------------------------------------------------------------
    def flush(self) -> int:
        """Sends the pending points that fit into the ring, in ONE stream_append; returns how many went."""
        m = min(len(self._pending), self.capacity - self.retained)
        if m <= 0:
            return 0
        arrays = self.point_arrays(self._pending[:m])
        self._hip.stream_append(*arrays)
        del self._pending[:m]
        self._end += m
        return m

    def point_arrays(self, items):
        """(q, dq, ddq [B][m][nv], pose [B][m][12], w_pose [B][m][6], w_collision [B][m] or None) of m items: the arguments of
        `HipOcp.stream_append`, read from the points the way OCPCrocoGeneric.set_reference_weighted_trajectory reads them."""
        B, nv, m = self.B, self.nv, len(items)
        q, dq, ddq = np.zeros((B, m, nv)), np.zeros((B, m, nv)), np.zeros((B, m, nv))
        pose, w_pose, w_coll = np.empty((B, m, 12)), np.empty((B, m, 6)), np.empty((B, m))
        n_coll = 0
        for j, pts in enumerate(items):
            for b, wp in enumerate(pts):
                p, w = wp.point, wp.weights
                q[b, j] = np.asarray(p.robot_configuration, dtype=np.float64).reshape(nv)
                dq[b, j] = np.asarray(p.robot_velocity, dtype=np.float64).reshape(nv)
                if p.robot_acceleration is not None:
                    ddq[b, j] = np.asarray(p.robot_acceleration, dtype=np.float64).reshape(nv)
                pose[b, j] = as_se3_12(p.end_effector_poses[self.frame])
                w_pose[b, j] = _vec(w.w_end_effector_poses[self.frame], 6)
                if w.w_collision_avoidance is not None:
                    w_coll[b, j] = float(w.w_collision_avoidance)
                    n_coll += 1
        if n_coll not in (0, B * m):
            raise ValueError("w_collision_avoidance is set on some of the appended points only: give it on all of them or on none")
        return q, dq, ddq, pose, w_pose, (w_coll if n_coll else None)

    # -- helpers -------------------------------------------------------------------
    def _as_instance_points(self, item):
        if isinstance(item, WeightedTrajectoryPoint):
            if self.B != 1:
                raise ValueError(f"a handle of {self.B} instances takes {self.B} points per sample, got one")
            return [item]
        pts = list(item)
        if len(pts) != self.B or not all(isinstance(p, WeightedTrajectoryPoint) for p in pts):
            raise ValueError(f"expected {self.B} WeightedTrajectoryPoints per sample")
        return pts

    def _check_joint_weights(self, wp: WeightedTrajectoryPoint, b: int):
        w = wp.weights
        for name, got, want in (("w_robot_configuration", w.w_robot_configuration, self.w_q), ("w_robot_velocity", w.w_robot_velocity, self.w_qdot),
                                ("w_robot_effort", w.w_robot_effort, self.w_effort)):  # fmt: skip
            if got is None or not np.array_equal(_vec(got, self.nv), want):
                raise ValueError(f"instance {b}: {name} = {got} differs from the joint weights the streamed trajectory was created with "
                                 f"({want}): the ring holds them per handle")


class StreamedMPC:
    """`MPC` (mpc.py) on a `DeviceTrajectoryBuffer`: reference update, warm start, solve and shift are one `HipOcp.mpc_step` on the
    ring.  `run` returns the first node of the solution -- states [x0, x1], ricatti_gains [K0], feed_forward_terms [us0], what
    the controller publishes -- without a batch axis for B = 1, with one for B > 1."""

    def __init__(self) -> None:
        self._hip = None
        self._buffer: DeviceTrajectoryBuffer = None
        self._max_iter = 0
        self._started = False
        self._mpc_debug_data: MPCDebugData = None

    def setup(self, hip, buffer: DeviceTrajectoryBuffer, max_iter: int) -> None:
        self._hip, self._buffer, self._max_iter = hip, buffer, int(max_iter)
        self._started = False
        self._mpc_debug_data = MPCDebugData(ocp=OCPDebugData())

    def run(self, initial_state, current_time_ns: int = 0) -> OCPResults:
        """`initial_state`: a TrajectoryPoint (B = 1), B of them, or an array [B][nx] of measured states.  None while fewer than
        horizon_indexes[-1] + 1 samples are retained.  The first run starts from the reference (state and warm start of the
        window, as `mpc_step(first=1)` does), the later ones from the measured state and the shifted previous solution."""
        assert self._hip is not None and self._buffer is not None
        t_begin = time.perf_counter_ns()
        buf, hip = self._buffer, self._hip
        buf.flush()
        if buf.retained < buf.max_span:
            return None
        t_refs = time.perf_counter_ns()
        hip.upload_x0(self._state_array(initial_state))
        k0 = buf.first
        ref_id = buf.reference_id(0)
        hip.mpc_step(k0, self._max_iter, first=2 if self._started else 1)
        self._started = True
        us0, K0, x1, st = hip.download_first()
        x0 = hip.download_x0()
        buf.clear_past()
        one = hip.B == 1
        pick = (lambda a: a[0]) if one else (lambda a: a)
        res = OCPResults(states=[pick(x0), pick(x1)], ricatti_gains=[pick(K0)], feed_forward_terms=[pick(us0)])
        t_end = time.perf_counter_ns()
        dbg = self._mpc_debug_data
        dbg.ocp = OCPDebugData(result=res, kkt_norm=pick(st["kkt"]), nb_iter=pick(st["iter"]), nb_qp_iter=pick(st["qp_iters"]),
                               problem_solved=bool(np.all(st["solved"])))  # fmt: skip
        dbg.reference_id = ref_id
        dbg.duration_iteration_ns = t_end - t_begin
        dbg.duration_horizon_update_ns = t_refs - t_begin
        dbg.duration_generate_warm_start_ns = 0  # part of the device step
        dbg.duration_ocp_solve_ns = t_end - t_refs
        return res

    @property
    def mpc_debug_data(self) -> MPCDebugData:
        return self._mpc_debug_data

    def append_trajectory_point(self, trajectory_point):
        self._buffer.append(trajectory_point)

    def append_trajectory_points(self, trajectory_points):
        self._buffer.extend(trajectory_points)

    def _state_array(self, initial_state) -> np.ndarray:
        B = self._hip.B
        if isinstance(initial_state, TrajectoryPoint):
            initial_state = [initial_state]
        if isinstance(initial_state, (list, tuple)) and all(isinstance(s, TrajectoryPoint) for s in initial_state):
            initial_state = np.array([s.robot_state for s in initial_state])
        return np.asarray(initial_state, dtype=np.float64).reshape(B, self._hip.nx)
