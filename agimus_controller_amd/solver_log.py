"""Per-iteration solver log: what `OCPParamsBaseCroco.callbacks` gives upstream
(agimus_controller/agimus_controller/ocp_base_croco.py:77-80 installs mim_solvers.CallbackVerbose and CallbackLogger).

The records are written on the device while the solve runs (`HipOcp.iter_log`, agx_ocp_iter_log) and read afterwards, so the
table is available -- and printed by `OCPBaseCroco.solve` -- AFTER the solve, not line by line as the solve runs.

Columns of the table are those of CallbackVerbose
    iter  merit  cost  ||gaps||  ||Constraint||  ||(dx,du)||  step  KKT criteria  QP iters
minus ||(dx,du)||: the norm of the direction is not kept on the device.  CallbackLogger's history of xs / us is not kept
either.  `format(details=True)` adds what only this solver knows: the regularisation the direction was computed with, the step
lengths tried, and whether the direction was discarded or every step length rejected.
"""

from __future__ import annotations

import dataclasses

import numpy as np

from . import _abi

_FIELDS = tuple(_abi.ITER_RECORD_DTYPE.names)


@dataclasses.dataclass
class SolverLog:
    """Arrays per field, [B][n_max] with n_max = min(max(n), capacity); entries of instance b at or beyond min(n[b], capacity)
    are NaN (floats) / -1 (integers).  n [B]: SQP iterations every instance started; `capacity`: records kept per instance --
    where n[b] exceeds it the later iterations were dropped."""

    n: np.ndarray
    capacity: int
    kkt: np.ndarray
    cost: np.ndarray
    merit: np.ndarray
    gap_norm: np.ndarray
    constraint_norm: np.ndarray
    step: np.ndarray
    preg: np.ndarray
    dreg: np.ndarray
    iter: np.ndarray
    qp_iters: np.ndarray
    trials: np.ndarray
    flags: np.ndarray

    @classmethod
    def from_records(cls, records: np.ndarray, n: np.ndarray) -> "SolverLog":
        """`records` [B][capacity] of _abi.ITER_RECORD_DTYPE and `n` [B], as HipOcp.read_iter_log returns them."""
        records = np.asarray(records)
        n = np.asarray(n, dtype=np.int32).reshape(-1)
        if records.ndim != 2 or records.shape[0] != n.size:
            raise ValueError(f"records: expected shape ({n.size}, capacity), got {records.shape}")
        cap = records.shape[1]
        kept = np.minimum(n, cap)
        n_max = int(kept.max()) if kept.size else 0
        valid = np.arange(n_max)[None, :] < kept[:, None]
        cols = {}
        for name in _FIELDS:
            col = records[name][:, :n_max]
            fill = np.nan if col.dtype.kind == "f" else -1
            cols[name] = np.where(valid, col, fill).astype(col.dtype)
        return cls(n=n.copy(), capacity=cap, **cols)

    def kept(self, b: int = 0) -> int:
        """Records kept of instance b."""
        return int(min(self.n[b], self.capacity))

    def format(self, b: int = 0, details: bool = False) -> str:
        """The table of instance b, one line per SQP iteration, under CallbackVerbose's header (without ||(dx,du)||).  The
        converging iteration and an iteration without a step show step 0."""
        head = f"{'iter':>4}  {'merit':>12}  {'cost':>12}  {'||gaps||':>12}  {'||Constraint||':>14}  {'step':>8}  {'KKT criteria':>12}  {'QP iters':>8}"
        if details:
            head += f"  {'preg':>8}  {'dreg':>8}  {'trials':>6}  note"
        lines = [head]
        for j in range(self.kept(b)):
            line = (f"{int(self.iter[b, j]):4d}  {self.merit[b, j]:12.5e}  {self.cost[b, j]:12.5e}  {self.gap_norm[b, j]:12.5e}  "
                    f"{self.constraint_norm[b, j]:14.5e}  {self.step[b, j]:8.4f}  {self.kkt[b, j]:12.5e}  {int(self.qp_iters[b, j]):8d}")  # fmt: skip
            if details:
                f = int(self.flags[b, j])
                notes = [text for bit, text in ((_abi.ITER_CONVERGED, "converged"), (_abi.ITER_DISCARDED, "direction discarded"),
                                                (_abi.ITER_REJECTED, "all step lengths rejected"), (_abi.ITER_CUT, "cut before the search")) if f & bit]  # fmt: skip
                line += f"  {self.preg[b, j]:8.1e}  {self.dreg[b, j]:8.1e}  {int(self.trials[b, j]):6d}  {', '.join(notes)}"
            lines.append(line.rstrip())
        if self.n[b] > self.capacity:
            lines.append(f"... {int(self.n[b]) - self.capacity} more iterations not kept (capacity {self.capacity})")
        return "\n".join(lines)
