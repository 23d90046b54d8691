"""Streamed resident trajectory, the parts that need no GPU: the slot arithmetic of the ring with a mirrored tail
(`_abi.ring_slots`, the pure-Python mirror of k_traj_append's), `DeviceTrajectoryBuffer` against a fake backend that records the
calls, and the presence of the four entry points in the header, the symbol list and the generated front."""
import importlib.util
import pathlib

import numpy as np
import pytest

from agimus_controller_amd import _abi, backend
from agimus_controller_amd.factory import robot_tables as rt
from agimus_controller_amd.factory.robot_model import panda_robot_models
from agimus_controller_amd.ocp import ocp_croco_generic as g
from agimus_controller_amd.ocp_param_base import DTFactorsNSeq
from agimus_controller_amd.se3 import as_se3_12
from agimus_controller_amd.trajectory import TrajectoryPoint, TrajectoryPointWeights, WeightedTrajectoryPoint
from agimus_controller_amd.trajectory_stream import DeviceTrajectoryBuffer, StreamedMPC

ROOT = pathlib.Path(__file__).resolve().parents[1]
STREAM_SYMBOLS = ["agx_traj_stream_create", "agx_traj_stream_append", "agx_traj_stream_release", "agx_traj_stream_range",
                  "agx_traj_stream_joins", "agx_traj_stream_timing"]


# ---------------------------------------------------------------------------------------------------------- slot arithmetic
@pytest.mark.parametrize("C,span", [(8, 6), (12, 10)])
def test_ring_slots(C, span):
    M = span - 1
    for k in range(3 * C + 1):
        slot, mirror = _abi.ring_slots(k, C, span)
        assert slot == k % C and 0 <= slot < C
        assert mirror == (C + slot if slot < M else None)
        assert mirror is None or C <= mirror < C + M
    with pytest.raises(ValueError):
        _abi.ring_slots(0, 5, 6)
    with pytest.raises(ValueError):
        _abi.ring_slots(-1, 8, 6)


@pytest.mark.parametrize("C,span", [(8, 6), (12, 10)])
def test_every_window_is_contiguous_and_appends_never_touch_retained_samples(C, span):
    """A model of the device memory: cell -> logical sample written there last.  For every `first` the ring is filled to
    [first, first + C) the way the kernel writes it (slot and mirror slot); every window of `span` samples inside must read its
    samples from consecutive cells starting at k0 mod C.  Then every k in [end, first + C) for every shorter retained range: the
    cells an append of k writes hold no retained sample."""
    for first in range(2 * C + 1):
        cells = {}
        for k in range(max(0, first - C), first + C):  # older laps first: what the ring went through
            slot, mirror = _abi.ring_slots(k, C, span)
            cells[slot] = k
            if mirror is not None:
                cells[mirror] = k
        for k0 in range(first, first + C - span + 1):
            start = k0 % C
            assert start + span <= C + span - 1  # inside the allocation
            assert [cells[start + t] for t in range(span)] == list(range(k0, k0 + span)), (first, k0)
        for end in range(first, first + C + 1):
            retained_cells = set()
            for k in range(first, end):
                retained_cells.update(c for c in _abi.ring_slots(k, C, span) if c is not None)
            for k in range(end, first + C):
                new = {c for c in _abi.ring_slots(k, C, span) if c is not None}
                assert not (new & retained_cells), (first, end, k)


# ---------------------------------------------------------------------------------------------- DeviceTrajectoryBuffer
class FakeHip:
    """Stands where a HipOcp stands and records the calls."""

    def __init__(self, table, B, T):
        self.table, self.B, self.T = table, B, T
        self.nv, self.nx = table.nv, 2 * table.nv
        self.calls = []
        self.first = self.end = 0
        self.capacity = None

    def stream_trajectory(self, capacity, max_span, w_q, w_qdot, w_effort, w_pose, frame):
        self.capacity = capacity
        self.calls.append(("create", capacity, max_span, np.array(w_q), np.array(w_qdot), np.array(w_effort), np.array(w_pose), frame))

    def set_horizon_indexes(self, idx):
        self.calls.append(("hidx", list(idx)))

    def stream_append(self, q, dq, ddq, pose=None, w_pose=None, w_collision=None):
        assert self.end + q.shape[1] - self.first <= self.capacity
        self.end += q.shape[1]
        self.calls.append(("append", q.copy(), dq.copy(), ddq.copy(), pose, w_pose, w_collision))

    def stream_release(self, k):
        assert self.first <= k <= self.end
        self.first = k
        self.calls.append(("release", k))

    def named(self, name):
        return [c for c in self.calls if c[0] == name]


W_Q, W_QDOT, W_EFF = np.full(7, 1.5), np.full(7, 0.2), np.full(7, 1e-3)


def _point(rng, i, frame="panda_hand_tcp", w_q=W_Q, w_coll=0.25, short_weights=False):
    R = rt.rpy(*rng.uniform(-1, 1, 3))
    from agimus_controller_amd.se3 import SE3

    pt = TrajectoryPoint(id=i, time_ns=i, robot_configuration=rng.uniform(-1, 1, 7), robot_velocity=rng.uniform(-1, 1, 7),
                         robot_acceleration=rng.uniform(-1, 1, 7), robot_effort=rng.uniform(-1, 1, 7),
                         end_effector_poses={frame: SE3(R, rng.uniform(-0.5, 0.5, 3))})
    w = TrajectoryPointWeights(w_robot_configuration=np.array([1.5]) if short_weights else w_q.copy(), w_robot_velocity=W_QDOT.copy(),
                               w_robot_acceleration=np.zeros(7), w_robot_effort=W_EFF.copy(),
                               w_end_effector_poses={frame: rng.uniform(0.1, 2.0, 6)}, w_collision_avoidance=w_coll)
    return WeightedTrajectoryPoint(pt, w)


def _buffer(B=1, capacity=8, seq=None):
    seq = seq or DTFactorsNSeq(factors=[1], n_steps=[3])
    T = sum(seq.n_steps)
    hip = FakeHip(rt.panda_table(0.1), B, T)
    return hip, DeviceTrajectoryBuffer(hip, seq, capacity, "panda_hand_tcp", W_Q, W_QDOT, W_EFF)


def test_buffer_creates_the_ring_with_the_horizon_indexes_of_the_reference_buffer():
    hip, buf = _buffer(seq=DTFactorsNSeq(factors=[1, 2, 3], n_steps=[2, 2, 1]), capacity=12)
    assert buf.horizon_indexes == [0, 1, 2, 4, 6, 9] and buf.max_span == 10
    kind, capacity, max_span, w_q, w_qdot, w_eff, w_pose, frame = hip.named("create")[0]
    assert (capacity, max_span, frame) == (12, 10, hip.table.frame_id("panda_hand_tcp"))
    assert np.array_equal(w_q, W_Q) and np.array_equal(w_qdot, W_QDOT) and np.array_equal(w_eff, W_EFF)
    assert hip.named("hidx") == [("hidx", [0, 1, 2, 4, 6, 9])]
    assert len(buf) == 0


def test_point_arrays_are_what_set_reference_weighted_trajectory_reads():
    """The arrays of one stream_append against the `update()` of the residual classes, which is how
    OCPCrocoGeneric.set_reference_weighted_trajectory (`_update_node`) reads a point."""
    rng = np.random.default_rng(0)
    hip, buf = _buffer()
    pts = [_point(rng, i, short_weights=(i == 1)) for i in range(4)]
    buf.extend(pts)
    assert buf.flush() == 4
    (_, q, dq, ddq, pose, w_pose, w_coll), = hip.named("append")
    assert q.shape == (1, 4, 7) and pose.shape == (1, 4, 12) and w_pose.shape == (1, 4, 6) and w_coll.shape == (1, 4)
    data = g.BuildData(panda_robot_models().robot_model, 7)
    for j, wp in enumerate(pts):
        x, w_x, _ = g.ResidualModelState().update(data, wp)
        assert np.array_equal(np.concatenate([q[0, j], dq[0, j]]), x)
        assert np.array_equal(w_x, np.concatenate([W_Q, W_QDOT]))  # the per-handle joint weights are the point's
        ref, w, frame = g.ResidualModelFramePlacement(id="panda_hand_tcp").update(data, wp)
        assert np.array_equal(pose[0, j], ref) and np.array_equal(pose[0, j], as_se3_12(wp.point.end_effector_poses["panda_hand_tcp"]))
        assert np.array_equal(w_pose[0, j], g._vec(w, 6))
        assert frame == buf.frame_id
        assert np.array_equal(ddq[0, j], wp.point.robot_acceleration)
        assert w_coll[0, j] == float(wp.weights.w_collision_avoidance)


def test_appends_are_batched_and_clear_past_releases():
    rng = np.random.default_rng(1)
    hip, buf = _buffer(capacity=5)
    pts = [_point(rng, i) for i in range(9)]
    buf.append(pts[0])
    buf.append(pts[1])
    buf.extend(pts[2:4])
    assert len(buf) == 4 and buf.retained == 0 and not hip.named("append")  # nothing sent before a flush
    assert buf.flush() == 4 and len(hip.named("append")) == 1 and hip.named("append")[0][1].shape == (1, 4, 7)
    assert (hip.first, hip.end, buf.retained, len(buf)) == (0, 4, 4, 4)
    assert buf.flush() == 0 and len(hip.named("append")) == 1
    # more than fits: the rest stays pending (the buffer is unbounded) and goes once the past is released
    buf.extend(pts[4:9])
    assert len(buf) == 9
    assert buf.flush() == 1 and (buf.retained, len(buf)) == (5, 9)
    buf.clear_past()
    assert hip.named("release") == [("release", 1)] and (buf.first, buf.retained, len(buf)) == (1, 4, 8)
    assert buf.reference_id(0) == 1
    buf.clear_past()
    assert hip.named("release")[-1] == ("release", 2)
    assert buf.flush() == 2 and hip.named("append")[-1][1].shape == (1, 2, 7)
    assert np.array_equal(hip.named("append")[-1][1][0, 0], pts[5].point.robot_configuration)
    assert (hip.first, hip.end) == (2, 7) and len(buf) == 7
    # clear_past on a buffer whose points are all pending sends them first
    hip2, buf2 = _buffer()
    buf2.append(pts[0])
    buf2.clear_past()
    assert [c[0] for c in hip2.calls[2:]] == ["append", "release"] and len(buf2) == 0
    buf2.clear_past()  # empty: nothing happens, as in TrajectoryBuffer
    assert len(hip2.named("release")) == 1


def test_batch_of_point_lists():
    rng = np.random.default_rng(2)
    hip, buf = _buffer(B=3)
    items = [[_point(rng, 10 * j + b) for b in range(3)] for j in range(2)]
    buf.extend(items)
    buf.flush()
    q = hip.named("append")[0][1]
    assert q.shape == (3, 2, 7)
    for j in range(2):
        for b in range(3):
            assert np.array_equal(q[b, j], items[j][b].point.robot_configuration)
    with pytest.raises(ValueError, match="3 points per sample"):
        buf.append(items[0][0])
    with pytest.raises(ValueError, match="expected 3 WeightedTrajectoryPoints"):
        buf.append(items[0][:2])


def test_changed_joint_weights_are_refused():
    rng = np.random.default_rng(3)
    hip, buf = _buffer()
    buf.append(_point(rng, 0))
    with pytest.raises(ValueError, match="w_robot_configuration.*differs from the joint weights"):
        buf.append(_point(rng, 1, w_q=np.full(7, 2.0)))
    assert len(buf) == 1
    # the collision weight on some points only
    buf.append(_point(rng, 2, w_coll=None))
    with pytest.raises(ValueError, match="w_collision_avoidance is set on some"):
        buf.flush()


def test_streamed_mpc_waits_for_a_full_window():
    rng = np.random.default_rng(4)
    hip, buf = _buffer()  # T = 3: four samples make a window
    mpc = StreamedMPC()
    mpc.setup(hip, buf, 5)
    state = _point(rng, 0).point
    for i in range(3):
        mpc.append_trajectory_point(_point(rng, i))
        assert mpc.run(state, 0) is None
    assert buf.retained == 3 and not hip.named("release")


# ------------------------------------------------------------------------------------------------------------------ ABI
def test_the_entry_points_are_declared_exported_and_forwarded():
    hdr = (ROOT / "include" / "agimus_hip.h").read_text()
    spec = importlib.util.spec_from_file_location("agx_front", ROOT / "agimus_controller_amd" / "csrc" / "agx_front.py")
    front = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(front)
    declared = {name: params for _, name, params in front.prototypes(hdr)}
    src = front.front_source(hdr)
    for name in STREAM_SYMBOLS:
        assert name in backend.EXPORTED_SYMBOLS
        assert name in declared and "agx_ocp" in declared[name][0][0]
        assert f"int {name}(" in src and f"{name}_g0(" in src and f"{name}_g1(" in src
    backend.build()
    for name in STREAM_SYMBOLS:
        assert hasattr(backend.lib(), name)
