"""Cartesian sine wave tracked with a pose weight that grows over every half cycle
(trajectories/sine_wave_cartesian_space_weight_increasing.py:19-108 upstream): joint positions, velocities and efforts follow
the sine through the inverse kinematics of the parent class, while the end-effector target jumps between the two extrema of
the sine and its translational weight ramps up (WeightIncreasing) with the time spent heading for the current extremum.
`HipOcp.cartesian_sine_weight_increasing_trajectory` builds the same schedule on the device."""

from __future__ import annotations

from copy import deepcopy

import numpy as np

from ..se3 import SE3ToXYZQUAT
from ..trajectory import TrajectoryPoint, TrajectoryPointWeights, WeightedTrajectoryPoint
from .sine_wave_cartesian_space import SinusWaveCartesianSpace
from .sine_wave_params import SinWaveParams
from .weight_increasing import WeightIncreasing


class SinusWaveCartesianSpaceWeightIncreasing(SinusWaveCartesianSpace):
    """Sine wave in cartesian space whose end-effector cost weight increases over time within a cycle."""

    def __init__(self, sine_wave_params: SinWaveParams, w_increasing: WeightIncreasing, ee_frame_name, w_q, w_qdot, w_qddot,
                 w_robot_effort, w_pose, mask=(True, True, True, True, True, True)):  # fmt: skip
        super().__init__(sine_wave_params, ee_frame_name, w_q, w_qdot, w_qddot, w_robot_effort, w_pose, mask)
        self.w_increasing = w_increasing
        self.cycle_durations = sine_wave_params.period

    def get_targets_time(self, t, cycle_duration):
        """(t1, t2): time since the running cycle began and the same instant half a cycle away.  The device kernel repeats
        these operations one by one (quotient, truncation, product, difference), so both agree on which is smaller."""
        cycle_start_time = int(t / cycle_duration) * cycle_duration
        time_target_1 = t - cycle_start_time
        if time_target_1 > cycle_duration:
            time_target_1 -= cycle_duration
        half = cycle_duration / 2.0
        time_target_2 = time_target_1 + half if time_target_1 < half else time_target_1 - half
        return (time_target_1, time_target_2)

    def get_traj_point_at_t(self, t) -> WeightedTrajectoryPoint:
        quint, dquint, _ = self.quint_traj.get_value_at_t(t)
        sin_wt, cos_wt = np.sin(self.w * t), np.cos(self.w * t)
        ee_des_vel = np.zeros(6)
        ee_des_vel[:3] = self.amp * (dquint * sin_wt + quint * self.w * cos_wt)

        # joints: inverse kinematics of the sine itself, as in the parent class
        sine_pose = self.ee_init_pos.copy()
        sine_pose.translation = sine_pose.translation + self.amp * quint * sin_wt
        q, dq = self.inverse_kinematics(sine_pose, ee_des_vel)

        # end effector: per axis the extremum the sine is heading for, weighted by the time spent on the way
        ee_des_pos = self.ee_init_pos.copy()
        w_pose = self.w_pose  # upstream writes the first three entries of the constructor's array in place; kept visible
        for ax in range(3):
            t1, t2 = self.get_targets_time(t, self.cycle_durations[ax])
            sign = 1.0 if t1 < t2 else -1.0
            ee_des_pos.translation[ax] = ee_des_pos.translation[ax] + sign * (self.amp[ax] * quint[ax])
            w_pose[ax] = self.w_increasing.get_weight_at_t(max(t1, t2))

        u = self._dyn.rnea(q, dq, self.ddq)[0]
        traj_point = TrajectoryPoint(time_ns=t, robot_configuration=q, robot_velocity=dq, robot_acceleration=self.ddq, robot_effort=u,
                                     end_effector_poses={self.ee_frame_name: SE3ToXYZQUAT(ee_des_pos)})  # fmt: skip
        traj_weights = TrajectoryPointWeights(w_robot_configuration=self.w_q, w_robot_velocity=self.w_qdot,
                                              w_robot_acceleration=self.w_qddot, w_robot_effort=self.w_robot_effort,
                                              w_end_effector_poses={self.ee_frame_name: w_pose})  # fmt: skip
        return WeightedTrajectoryPoint(point=deepcopy(traj_point), weights=deepcopy(traj_weights))
