"""Cost weight that grows with time along a hyperbolic tangent (trajectories/weight_increasing.py:4-20 upstream):
w(t) = max_weight tanh(t arctanh(percent) / time_reach_percent), so w(0) = 0, w(time_reach_percent) = percent max_weight
and w -> max_weight."""

from __future__ import annotations

import numpy as np


class WeightIncreasing:
    def __init__(self, max_weight: float, percent: float, time_reach_percent: float):
        self.max_weight = max_weight
        self.percent = percent
        self.time_reach_percent = time_reach_percent

    @property
    def rate(self) -> float:
        """arctanh(percent) / time_reach_percent: the device generators evaluate max_weight tanh(rate t)."""
        return float(np.arctanh(self.percent) / self.time_reach_percent)

    def get_weight_at_t(self, t):
        return self.max_weight * np.tanh(t * np.arctanh(self.percent) / self.time_reach_percent)
