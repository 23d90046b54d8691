"""User-fed trajectory with a visual-servoing phase (trajectories/generic_visual_servoing_trajectory.py:11-145 upstream): inside
`visual_servoing_idx_range` the pose weight of the "<ee>_vs" frame ramps up (WeightIncreasing) and the collision-avoidance weight
takes its visual-servoing value; afterwards the ramp is walked back until the weight is zero again.
`schedule_arrays` evaluates the whole schedule at once for `HipOcp.generic_trajectory_weighted`, which keeps it on the device."""

from __future__ import annotations

import copy
from enum import Enum

import numpy as np

from ..se3 import SE3, SE3ToXYZQUAT, XYZQUATToSE3, as_se3_12
from ..trajectory import TrajectoryPointWeights, WeightedTrajectoryPoint
from .generic_trajectory import GenericTrajectory
from .weight_increasing import WeightIncreasing


class VisualServoingState(Enum):
    """Possible states for visual servoing."""

    IDLE = 1
    USING_VISUAL_SERVOING = 2
    COMING_BACK_TO_IDLE = 3


class GenericVisualServoingTrajectory(GenericTrajectory):
    """Trajectory fed by the user that can enable visual servoing."""

    def __init__(self, ee_frame_name, traj_params, dt, w_q, w_qdot, w_qddot, w_robot_effort, w_pose, w_increasing: WeightIncreasing,
                 w_collision_avoidance):  # fmt: skip
        super().__init__(ee_frame_name, w_q, w_qdot, w_qddot, w_robot_effort, w_pose, w_collision_avoidance)
        self.w_pose_constant = w_pose
        self.w_increasing = w_increasing
        self.w_increasing_max_rotation = traj_params.w_increasing_max_rotation
        self.w_increasing_max_collision_avoidance = traj_params.w_increasing_max_collision_avoidance
        self.visual_servoing_state = VisualServoingState.IDLE
        self.dt = dt
        self.visual_servoing_time = 0.0
        self.init_in_world_M_object = None
        self.robot_frame = self.ee_frame_name + "_vs"
        self.w_collision_avoidance = w_collision_avoidance
        # indexes of the current trajectory between which visual servoing is on: [first, last)
        self.visual_servoing_idx_range = (0, 0)

    def update_activation_of_visual_servoing(self):
        """One transition of the state machine, from the index of the point about to be handed out."""
        first, last = self.visual_servoing_idx_range
        if first <= self.traj_idx < last:
            if self.visual_servoing_state != VisualServoingState.USING_VISUAL_SERVOING:
                self.visual_servoing_time = 0.0
            self.visual_servoing_state = VisualServoingState.USING_VISUAL_SERVOING
        elif self.visual_servoing_time > 0.0:
            self.visual_servoing_state = VisualServoingState.COMING_BACK_TO_IDLE
        else:
            self.visual_servoing_state = VisualServoingState.IDLE

    def add_trajectory(self, trajectory, visual_servoing_idx_range, init_in_world_M_object=None):
        if init_in_world_M_object is None and visual_servoing_idx_range[0] != visual_servoing_idx_range[1]:
            raise ValueError("Init pose detection not set.")
        if init_in_world_M_object is not None:
            self.init_in_world_M_object = XYZQUATToSE3(init_in_world_M_object)
        super().add_trajectory(trajectory)
        self.visual_servoing_idx_range = visual_servoing_idx_range
        self.traj_idx = 0
        self.trajectory = trajectory  # the new trajectory replaces the stored one (and is the caller's list, not a copy)

    def _ramped_weights(self):
        w = self.w_increasing.get_weight_at_t(self.visual_servoing_time)
        w_rot = w * self.w_increasing_max_rotation / self.w_increasing.max_weight
        w_collision = self.w_increasing_max_collision_avoidance * self.w_increasing_max_rotation / self.w_increasing.max_weight
        return [w] * 3 + [w_rot] * 3, w_collision

    def get_traj_point_at_t(self, t) -> WeightedTrajectoryPoint:
        self.update_activation_of_visual_servoing()
        traj_point = self.trajectory[self.traj_idx]
        key = next(iter(traj_point.end_effector_poses))
        if self.init_in_world_M_object is not None:
            # As upstream, the STORED point is rewritten in place with the pose expressed in the object frame: a point handed
            # out twice (the last one, once the trajectory is done) is transformed twice.
            p = as_se3_12(traj_point.end_effector_poses[key])
            in_object_M_ee = self.init_in_world_M_object.inverse() * SE3(p[:9].reshape(3, 3), p[9:])
            traj_point.end_effector_poses[key] = SE3ToXYZQUAT(in_object_M_ee)
        if self.visual_servoing_state == VisualServoingState.USING_VISUAL_SERVOING:
            self.w_pose, w_collision_avoidance = self._ramped_weights()
            self.visual_servoing_time = min(self.visual_servoing_time + self.dt, self.w_increasing.time_reach_percent)
        elif self.visual_servoing_state == VisualServoingState.COMING_BACK_TO_IDLE:
            self.w_pose, w_collision_avoidance = self._ramped_weights()
            self.visual_servoing_time -= self.dt
        else:
            self.w_pose = np.zeros(6)
            w_collision_avoidance = self.w_collision_avoidance
        self.trajectory_is_done = self.traj_idx == len(self.trajectory) - 1
        self.traj_idx = min(self.traj_idx + 1, len(self.trajectory) - 1)
        traj_weights = TrajectoryPointWeights(
            w_robot_configuration=self.w_q, w_robot_velocity=self.w_qdot, w_robot_acceleration=self.w_qddot,
            w_robot_effort=self.w_robot_effort, w_end_effector_poses={self.robot_frame: self.w_pose},
            w_collision_avoidance=w_collision_avoidance)  # fmt: skip
        return WeightedTrajectoryPoint(point=traj_point, weights=traj_weights)

    def schedule_arrays(self):
        """The whole stored trajectory through the state machine, once, from its first point: (w_pose [n][6], w_collision [n],
        pose [n][12] as R row major | p) -- the per-sample arrays of `HipOcp.generic_trajectory_weighted`.  Works on a copy of
        the points and puts the state of the object back, so the trajectory can still be played afterwards."""
        keep = {k: getattr(self, k) for k in ("trajectory", "traj_idx", "visual_servoing_state", "visual_servoing_time", "w_pose",
                                              "trajectory_is_done")}  # fmt: skip
        n = len(self.trajectory)
        w_pose, w_collision, pose = np.empty((n, 6)), np.empty(n), np.empty((n, 12))
        try:
            self.trajectory = copy.deepcopy(self.trajectory)
            self.traj_idx, self.visual_servoing_state, self.visual_servoing_time = 0, VisualServoingState.IDLE, 0.0
            for i in range(n):
                wp = self.get_traj_point_at_t(i * self.dt)
                w_pose[i] = np.asarray(wp.weights.w_end_effector_poses[self.robot_frame], dtype=float)
                w_collision[i] = wp.weights.w_collision_avoidance
                pose[i] = as_se3_12(next(iter(wp.point.end_effector_poses.values())))
        finally:
            for k, v in keep.items():
                setattr(self, k, v)
        return w_pose, w_collision, pose
