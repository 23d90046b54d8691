"""The host side of the diagnostics, without a GPU: the record of the per-iteration solver log against the header, the table
`SolverLog.format` prints, and the arrays `cost_items` assembles out of `HipOcp.item_costs`."""
import ctypes as C
import pathlib
import re

import numpy as np

from agimus_controller_amd import _abi
from agimus_controller_amd.ocp.ocp_croco_generic import assemble_cost_items
from agimus_controller_amd.solver_log import SolverLog

ROOT = pathlib.Path(__file__).resolve().parents[1]


def test_iter_record_is_eighty_bytes_and_matches_the_header():
    hdr = (ROOT / "include" / "agimus_hip.h").read_text()
    body = re.search(r"typedef struct agx_iter_record \{(.*?)\} agx_iter_record;", hdr, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", " ", body, flags=re.S)
    declared = []
    for ctype, names in re.findall(r"\b(double|int32_t)\s+([^;]+);", body):
        declared += [(n.strip(), ctype) for n in names.split(",")]
    mirrored = [(n, "double" if t is C.c_double else "int32_t") for n, t in _abi.IterRecord._fields_]
    assert declared == mirrored
    assert C.sizeof(_abi.IterRecord) == _abi.ITER_RECORD_DTYPE.itemsize == 80
    for name, _ in declared:  # numpy and ctypes agree on every offset
        assert _abi.ITER_RECORD_DTYPE.fields[name][1] == getattr(_abi.IterRecord, name).offset


def _records():
    """Two instances, capacity 4: instance 0 converges in its third iteration after a backtracked and a full step; instance 1
    runs five iterations (one dropped): a discarded direction, a search that rejects all ten step lengths, then full steps."""
    rec = np.zeros((2, 4), dtype=_abi.ITER_RECORD_DTYPE)
    rows0 = [(3.0, 10.0, 12.0, 0.2, 0.0, 0.25, 1e-9, 1e-9, 0, 1, 3, 0), (0.5, 4.0, 4.5, 0.05, 0.0, 1.0, 1e-9, 1e-9, 1, 1, 1, 0),
             (1e-4, 3.5, 3.5, 0.0, 0.0, 0.0, 1e-9, 1e-9, 2, 1, 0, _abi.ITER_CONVERGED)]
    rows1 = [(np.nan, 8.0, 9.0, 0.1, 0.3, 0.0, 1e-9, 1e-9, 0, 17, 0, _abi.ITER_DISCARDED),
             (2.0, 8.0, 9.0, 0.1, 0.3, 0.0, 1e-8, 1e-8, 1, 20, 10, _abi.ITER_REJECTED),
             (2.0, 8.0, 9.0, 0.1, 0.3, 1.0, 1e-7, 1e-7, 2, 12, 1, 0), (1.0, 6.0, 6.5, 0.05, 0.0, 1.0, 1e-8, 1e-8, 3, 9, 1, 0)]
    for b, rows in enumerate((rows0, rows1)):
        for j, row in enumerate(rows):
            rec[b, j] = row
    return rec, np.array([3, 5], dtype=np.int32)


def test_solver_log_arrays_and_table():
    rec, n = _records()
    log = SolverLog.from_records(rec, n)
    assert log.capacity == 4 and list(log.n) == [3, 5] and log.kept(0) == 3 and log.kept(1) == 4
    assert log.kkt.shape == (2, 4) and log.flags.dtype == np.int32
    assert np.isnan(log.cost[0, 3]) and log.iter[0, 3] == -1 and log.trials[0, 3] == -1  # beyond n[0]
    np.testing.assert_array_equal(log.step[0, :3], [0.25, 1.0, 0.0])
    np.testing.assert_array_equal(log.qp_iters[1], [17, 20, 12, 9])
    lines = log.format(0).splitlines()
    assert lines[0].split() == ["iter", "merit", "cost", "||gaps||", "||Constraint||", "step", "KKT", "criteria", "QP", "iters"]
    assert "(dx,du)" not in lines[0]
    assert len(lines) == 1 + 3
    cells = lines[1].split()
    assert cells[0] == "0" and float(cells[1]) == 12.0 and float(cells[2]) == 10.0 and float(cells[3]) == 0.2
    assert float(cells[5]) == 0.25 and float(cells[6]) == 3.0 and cells[7] == "1"
    assert float(lines[3].split()[5]) == 0.0  # the converging iteration takes no step
    # the second instance: one line per record kept, and a note on the iteration that was dropped
    lines = log.format(1, details=True).splitlines()
    assert len(lines) == 1 + 4 + 1 and "1 more iterations not kept (capacity 4)" in lines[-1]
    assert lines[0].split()[-4:] == ["preg", "dreg", "trials", "note"]
    assert lines[1].endswith("direction discarded") and lines[2].endswith("all step lengths rejected")
    assert "nan" in lines[1].lower()  # the KKT residual of a discarded direction is undefined
    assert lines[2].split()[8:11] == ["1.0e-08", "1.0e-08", "10"]  # (eight columns of the table, then preg, dreg, trials)


def test_solver_log_of_a_solve_that_started_nothing():
    rec = np.zeros((1, 3), dtype=_abi.ITER_RECORD_DTYPE)
    log = SolverLog.from_records(rec, np.zeros(1, dtype=np.int32))
    assert log.kkt.shape == (1, 0) and len(log.format(0).splitlines()) == 1


def test_cost_items_name_union_and_nan_pattern():
    """A stub of HipOcp.item_costs: running items a, b, c and terminal items b, d on T = 3, nx = 4, nu = 2."""
    T_, nx, nu = 3, 4, 2
    rng = np.random.default_rng(0)
    items = {"cost_r": rng.normal(size=(1, T_, 3)), "Lx_r": rng.normal(size=(1, T_, 3, nx)), "Lu_r": rng.normal(size=(1, T_, 3, nu)),
             "cost_t": rng.normal(size=(1, 2)), "Lx_t": rng.normal(size=(1, 2, nx))}
    out = assemble_cost_items(["a", "b", "c"], ["b", "d"], items)
    assert out.names == ["a", "b", "c", "d"]  # first seen: the running nodes come first
    assert out.values.shape == (4, T_ + 1) and out.jacobian.shape == (4, (T_ + 1) * (nx + nu))
    nan = np.isnan(out.values)
    np.testing.assert_array_equal(nan, [[False] * 3 + [True], [False] * 4, [False] * 3 + [True], [True] * 3 + [False]])
    np.testing.assert_array_equal(out.values[1], np.append(items["cost_r"][0, :, 1], items["cost_t"][0, 0]))
    assert out.values[3, T_] == items["cost_t"][0, 1]
    jac = out.jacobian.reshape(4, T_ + 1, nx + nu)
    np.testing.assert_array_equal(jac[2, :T_, :nx], items["Lx_r"][0, :, 2])
    np.testing.assert_array_equal(jac[2, :T_, nx:], items["Lu_r"][0, :, 2])
    np.testing.assert_array_equal(jac[1, T_, :nx], items["Lx_t"][0, 0])
    assert not jac[:, T_, nx:].any()  # the terminal node has no control
    assert not jac[3, :T_].any() and not jac[0, T_].any()  # an item a node type lacks: zero gradient, NaN value
