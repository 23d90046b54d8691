"""Per-instance plant inertials and the model-sensitivity sweep: what needs no GPU (the table helpers of workloads.py,
the column order, the C ABI surface, and the reference construction the GPU tests build their expected matrix with)."""
import dataclasses
import pathlib
import re

import numpy as np

from agimus_controller_amd import _abi, backend, workloads
from agimus_controller_amd.factory import robot_tables as rt
from oracle.oracle import Oracle

ROOT = pathlib.Path(__file__).resolve().parents[1]


def test_plant_tables_entry_zero_is_the_input_and_shapes_are_right():
    table = rt.panda_table(0.1)
    tables = workloads.plant_tables(table, 5, seed=3)
    assert len(tables) == 5 and tables[0] is table
    mass, com, inertia, armature = workloads.stack_inertials(tables)
    assert mass.shape == (5, 7) and com.shape == (5, 7, 3) and inertia.shape == (5, 7, 9) and armature.shape == (5, 7)
    np.testing.assert_array_equal(mass[0], table.mass)
    np.testing.assert_array_equal(com[0], table.com)
    np.testing.assert_array_equal(inertia[0], table.inertia.reshape(7, 9))
    np.testing.assert_array_equal(armature, np.broadcast_to(table.armature, (5, 7)))
    for t in tables[1:]:  # only the inertials differ
        np.testing.assert_array_equal(t.placement, table.placement)
        np.testing.assert_array_equal(t.axis, table.axis)
        np.testing.assert_array_equal(t.parent, table.parent)
        assert not np.array_equal(t.mass, table.mass)


def test_plant_tables_are_seeded_and_stay_within_rel():
    table = rt.panda_table(0.1)
    a = workloads.stack_inertials(workloads.plant_tables(table, 6, seed=3, rel=0.05))
    b = workloads.stack_inertials(workloads.plant_tables(table, 6, seed=3, rel=0.05))
    c = workloads.stack_inertials(workloads.plant_tables(table, 6, seed=4, rel=0.05))
    for x, y in zip(a, b):
        np.testing.assert_array_equal(x, y)
    assert not np.array_equal(a[0][1:], c[0][1:])
    # the first entries do not depend on how many follow
    d = workloads.stack_inertials(workloads.plant_tables(table, 3, seed=3, rel=0.05))
    np.testing.assert_array_equal(d[2], a[2][:3])
    mass, com, inertia, _ = a
    assert np.all(np.abs(mass / table.mass - 1.0) <= 0.05 + 1e-15)
    assert np.all(np.abs(com - table.com) <= 0.05 * np.abs(table.com).max(axis=1)[None, :, None] + 1e-15)
    scale = np.abs(table.inertia.reshape(7, 9)).max(axis=1)
    assert np.all(np.abs(inertia - table.inertia.reshape(7, 9)) <= 0.05 * scale[None, :, None] + 1e-15)
    assert np.abs(mass[1:] / table.mass - 1.0).max() > 0.02  # and they do move


def test_perturbed_inertias_stay_symmetric():
    for table in (rt.panda_table(0.1), rt.tree_table(9, seed=2)):
        nv = table.nv
        tables = workloads.plant_tables(table, 4, seed=9, payload=(1.5, (0.02, -0.01, 0.1)))
        for t in tables[2:]:  # the seeded perturbations: exactly
            I = np.asarray(t.inertia).reshape(nv, 3, 3)
            np.testing.assert_array_equal(I, I.transpose(0, 2, 1))
            assert not np.array_equal(I, table.inertia.reshape(nv, 3, 3))
        I = np.asarray(tables[1].inertia).reshape(nv, 3, 3)  # the lumped payload: as symmetric as lump_inertia's sums leave it
        np.testing.assert_allclose(I, I.transpose(0, 2, 1), rtol=0, atol=1e-16 * np.abs(I).max())


def test_payload_entry_is_the_hand_computed_lump():
    table = rt.panda_table(0.1)
    m2, c2 = 2.0, np.array([0.0, 0.0, 0.1])
    t1 = workloads.plant_tables(table, 3, seed=1, payload=(m2, c2))[1]
    m1, c1, I1 = table.mass[6], table.com[6], table.inertia[6].reshape(3, 3)
    # parallel-axis theorem by hand: a point mass joins link 7
    m = m1 + m2
    c = (m1 * c1 + m2 * c2) / m
    I = I1.copy()
    for mi, ci in ((m1, c1), (m2, c2)):
        d = ci - c
        I = I + mi * (d @ d * np.eye(3) - np.outer(d, d))
    assert t1.mass[6] == m
    np.testing.assert_allclose(t1.com[6], c, rtol=0, atol=1e-16)
    np.testing.assert_allclose(t1.inertia[6].reshape(3, 3), I, rtol=1e-14, atol=1e-18)
    mm, cc, II = rt.lump_inertia(m1, c1, I1, m2, c2, np.zeros((3, 3)))
    assert mm == t1.mass[6] and np.array_equal(cc, t1.com[6]) and np.array_equal(II.reshape(9), t1.inertia[6])
    # the other links are the nominal ones
    np.testing.assert_array_equal(t1.mass[:6], table.mass[:6])
    np.testing.assert_array_equal(t1.inertia[:6], table.inertia[:6])
    # without a payload entry 1 is an ordinary perturbed table
    assert workloads.plant_tables(table, 3, seed=1)[1].mass[0] != table.mass[0]


def test_sensitivity_columns_follow_the_reference_script():
    cols = workloads.sensitivity_columns(7)
    assert len(cols) == 70
    for l in range(7):
        block = cols[10 * l:10 * l + 10]
        assert block[:6] == [("inertia", l, 0, 0), ("inertia", l, 1, 0), ("inertia", l, 1, 1), ("inertia", l, 2, 0), ("inertia", l, 2, 1),
                             ("inertia", l, 2, 2)]
        assert block[6:9] == [("com", l, 0), ("com", l, 1), ("com", l, 2)]
        assert block[9] == ("mass", l)
    # the script's own loops (evaluate_model_sensibility.py:99-119): inertia columns count up over row, col <= row
    k = 0
    for row in range(3):
        for col in range(row + 1):
            assert cols[k] == ("inertia", 0, row, col)
            k += 1
    assert len(workloads.sensitivity_columns(9)) == 90


def test_header_and_symbol_list_declare_the_new_entry_points():
    hdr = (ROOT / "include" / "agimus_hip.h").read_text()
    for name in ("agx_ocp_set_plant_inertials", "agx_model_sensitivity"):
        assert re.search(r"\bint\s+" + name + r"\s*\(\s*agx_ocp\s*\*", hdr), name
        assert name in backend.EXPORTED_SYMBOLS
    for method in ("set_plant_inertials", "clear_plant_inertials", "model_sensitivity"):
        assert callable(getattr(backend.HipOcp, method))


def test_golden_points_are_the_five_measured_samples():
    x, u = workloads.load_state_control_points(ROOT / "tests" / "golden" / "state_and_control_expe_data.yaml")
    assert x.shape == (5, 14) and u.shape == (5, 7)
    assert x[0, 0] == -0.01234266 and u[4, 6] == -0.8094384
    assert np.all(np.isfinite(x)) and np.all(np.isfinite(u))


def test_checker_reproduces_the_diagonal_quirk():
    """The expected matrix of the GPU tests moves a diagonal inertia entry by 2 delta (the script adds delta at [row][col]
    and at [col][row]).  The checker tells that apart from a move by delta: the accelerations differ by about a factor two."""
    table = rt.panda_table(0.1)
    x, u = workloads.load_state_control_points(ROOT / "tests" / "golden" / "state_and_control_expe_data.yaml")
    po = _abi.PackedOcp(7, [0.01], *workloads.regulation_rows())
    delta = 0.01
    quirk = workloads.perturb_inertial(table, ("inertia", 3, 0, 0), delta)
    assert abs(quirk.inertia[3, 0] - (table.inertia[3, 0] + 2 * delta)) < 1e-15
    once = table.inertia.copy()
    once[3, 0] += delta
    once = dataclasses.replace(table, inertia=once)
    a = {name: Oracle(t, po, 1).forward_dynamics(x[1, :7], x[1, 7:], u[1]) for name, t in (("base", table), ("quirk", quirk), ("once", once))}
    d2, d1 = a["quirk"] - a["base"], a["once"] - a["base"]
    assert np.abs(d1).max() > 1e-3  # the entry matters at this sample
    assert np.abs(d2 - d1).max() > 0.3 * np.abs(d1).max()
    # an off-diagonal entry moves both mirror entries by delta
    off = workloads.perturb_inertial(table, ("inertia", 3, 2, 1), delta).inertia[3].reshape(3, 3)
    base = table.inertia[3].reshape(3, 3)
    assert off[2, 1] == base[2, 1] + delta and off[1, 2] == base[1, 2] + delta
