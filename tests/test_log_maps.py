"""The checker's log maps against exact values (tests/golden/log_map_cases.npz, made by tests/golden/make_log_map_fixture.py with
mpmath): orc_log6 / orc_jlog6 on a grid of rotation angles that covers every threshold of the code, and one-node checker problems
with a FramePlacement and a FrameRotation row.  The HIP kernels and the checker state the same formulas, so parity between them
says nothing about the formulas; this file and tests/test_log_maps_gpu.py do.

Tolerance of every comparison: 1e-11 x scale + 1e-14 + 8 x floor.  The first two terms are the project's bound for kernel outputs
(test_derivative_tiles); scale is the largest entry of the reference AT THAT CASE OR NODE (not of the whole field: a node at
theta = 1e-6 is not measured against one at theta = 3).  floor is the fixture's: |well-conditioned float64 - mpmath| from the same
stored inputs.  The factor 8: a kinematic chain multiplies up to nv placements in another order than the reference.  Largest
floor in the fixture: 4.2e-15 (log6) and 2.8e-15 (Jlog6) on the grid, 4.8e-14 (residual) and 2.7e-14 (Jacobian) on the device
nodes -- all at pi - 1e-2 - 1e-4, the last angle of log3's first formula, where theta / sin theta amplifies by 1 / (pi - theta).

Near pi on a coordinate axis pinocchio's explicit formula gives the two vanishing components of w as sqrt of a difference of two
numbers near 1: good to pi sqrt(2 eps) = 7e-8 by construction.  Those (`loose` in the fixture, with everything they enter) are
asserted to 1e-7; the component along the axis and |w| to the ordinary bound."""
import ctypes as C
import importlib.util
import pathlib

import numpy as np
import pytest

from agimus_controller_amd import _abi
from oracle import oracle as orc
from oracle.oracle import Oracle

GOLDEN = pathlib.Path(__file__).resolve().parent / "golden"
DT = 0.01


def _generator():
    spec = importlib.util.spec_from_file_location("make_log_map_fixture", GOLDEN / "make_log_map_fixture.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


GEN = _generator()


@pytest.fixture(scope="module")
def cases():
    return dict(np.load(GOLDEN / "log_map_cases.npz"))


def tolerance(scale, floor):
    return 1e-11 * scale + 1e-14 + 8.0 * floor


def compare(got, want, floor, what, failures):
    """|got - want| <= tolerance(largest |want|, floor); prints the figures, appends to failures."""
    err, scale = float(np.abs(got - want).max()), float(np.abs(want).max())
    tol = tolerance(scale, floor)
    print(f"{what}: err {err:.3e} tol {tol:.3e} (scale {scale:.3e}, floor {floor:.1e})")
    if not err <= tol:
        failures.append(f"{what}: err {err:.3e} > {tol:.3e}")


def test_fixture_regenerates(cases):
    pytest.importorskip("mpmath", reason="mpmath is not installed: the fixture cannot be regenerated here")
    fresh = GEN.generate()
    assert sorted(fresh) == sorted(cases)
    for k in fresh:
        np.testing.assert_array_equal(fresh[k], cases[k], err_msg=k)


def test_grid_covers_the_thresholds_and_the_reference_is_well_conditioned(cases):
    th = cases["theta"]
    for lo, hi in ((0.0, 0.0), (0.5e-8, 1e-8), (1e-8, 1.5e-8), (0.5e-6, 1e-6), (1e-6, 2e-6), (0.5e-4, 1e-4), (1e-4, 2e-4),
                   (np.pi - 1e-2 - 2e-4, np.pi - 1e-2), (np.pi - 1e-2, np.pi - 1e-2 + 2e-4), (np.pi, np.pi)):
        for kind in (0, 1):
            if lo == np.pi and kind == 0:
                continue  # pi exactly is representable on a coordinate axis only
            assert np.any((th >= lo) & (th <= hi) & (cases["axis_kind"] == kind)), (lo, hi, kind)
    pn = np.linalg.norm(cases["M12"][:, 9:], axis=1)
    assert np.any(pn == 0.0) and np.any((pn > 5e-4) & (pn < 2e-3)) and np.any(pn > 0.4)
    # the condition on the reference: away from pi the floor is at most 1e-12 x scale (+ 1e-15, a tenth of the tolerance's absolute
    # term: the inputs have entries of size 1 whatever the size of the log, and a node at theta = 0 has scale 1e-17)
    away = np.pi - th >= 1e-3
    assert np.all(cases["floor_log6"][away] <= 1e-15 + 1e-12 * np.abs(cases["log6"][away]).max(1))
    assert np.all(cases["floor_jlog6"][away] <= 1e-15 + 1e-12 * np.abs(cases["jlog6"][away]).max((1, 2)))
    for name in GEN.DEVICE_MODELS:
        away = np.pi - cases["device_theta"] >= 1e-3
        assert np.all(cases[f"{name}_floor_r"][:, away] <= 1e-15 + 1e-12 * np.abs(cases[f"{name}_r"][:, away]).max(-1)), name
        assert np.all(cases[f"{name}_floor_J"][:, away] <= 1e-15 + 1e-12 * np.abs(cases[f"{name}_J"][:, away]).max((-1, -2))), name
        assert np.isfinite(cases[f"{name}_floor_r"]).all() and np.isfinite(cases[f"{name}_floor_J"]).all()


def test_checker_log6_and_jlog6_on_every_case(cases):
    lib = orc.lib()
    failures = []
    for i, (M, th) in enumerate(zip(cases["M12"], cases["theta"])):
        M = np.ascontiguousarray(M)
        r, J = np.empty(6), np.empty((6, 6))
        assert lib.orc_log6(M.ctypes.data_as(C.c_void_p), r.ctypes.data_as(C.c_void_p)) == 0
        assert lib.orc_jlog6(M.ctypes.data_as(C.c_void_p), J.ctypes.data_as(C.c_void_p)) == 0
        want, wantJ, loose = cases["log6"][i], cases["jlog6"][i], cases["loose"][i]
        what = f"case {i} theta {th:.9g} axis {'xyz'[0] if cases['axis_kind'][i] else 'generic'} |p| {np.linalg.norm(M[9:]):.1e}"
        compare(r[~loose], want[~loose], cases["floor_log6"][i], what + " log6", failures)
        compare(np.linalg.norm(r[3:]), np.linalg.norm(want[3:]), cases["floor_log6"][i], what + " |w|", failures)
        pn = float(np.linalg.norm(M[9:]))
        if loose.any():
            # the linear part is A p - w x p / 2 + beta (w.p) w: the loose components enter it times at most (1/2 + 2 beta pi) |p|
            bound = 1e-7 * (1.0 + 1.2 * pn)
            err = float(np.abs(r[loose] - want[loose]).max())
            print(f"{what} loose components: err {err:.3e} bound {bound:.1e}")
            if not err <= bound:
                failures.append(f"{what} loose components: err {err:.3e} > {bound:.1e}")
        if np.isnan(wantJ).any():
            assert th == np.pi and np.isfinite(J).all()  # no derivative at pi; the code returns the limit from below
            continue
        assert not J[3:, :3].any()
        if loose.any():
            # Jlog6 is quadratic in (w, p) with |dJ3/dw| <= 1/2 + 2 beta pi = 1.14 and the top-right block C J3, |C| <= (1 + |p|)
            bound = 4e-7 * (1.0 + pn)
            err = float(np.abs(J - wantJ).max())
            print(f"{what} Jlog6 (loose w): err {err:.3e} bound {bound:.1e}")
            if not err <= bound:
                failures.append(f"{what} Jlog6 (loose w): err {err:.3e} > {bound:.1e}")
        else:
            compare(J, wantJ, cases["floor_jlog6"][i], what + " Jlog6", failures)
    assert not failures, "\n" + "\n".join(failures)


# --------------------------------------------------------------------------------------------- nodes of the device cases
def row_problem(name, kind, cases, B=None):
    """(table, po, ref, xs, us) with the nodes of a device case: a zero-weight Control row (running), then the row `kind`
    (FramePlacement or FrameRotation) with unit item weight, the fixture's Mref and the activation weights e_(t mod nr) at node t."""
    table, frame = GEN.device_model(name)
    nv = table.nv
    q, Mref = cases[f"{name}_q"], cases[f"{name}_Mref"]
    B = q.shape[0] if B is None else B
    T = q.shape[1] - 1
    nref, nr = _abi.row_nref(kind, nv), _abi.row_nr(kind, nv)
    row = _abi.RowSpec(kind, frame=frame, name="log_row")
    po = _abi.PackedOcp(nv, [DT] * T, [_abi.RowSpec(_abi.RES_CONTROL, weight=0.0, name="no_control_cost"), row], [row])
    ref = po.new_ref_tile(B)
    for terminal, r in ((False, 1), (True, 0)):
        w, rf, aw = po.row_view(ref, terminal, r)
        nodes = slice(T, T + 1) if terminal else slice(0, T)
        w[...] = 1.0
        rf[...] = Mref[:B, nodes, :nref]
        aw[...] = np.eye(nr)[np.arange(T + 1) % nr][None, nodes]
    po.row_view(ref, False, 0)[0][...] = 0.0
    xs = np.concatenate([q[:B], np.zeros_like(q[:B])], axis=-1)
    return table, po, ref, xs, np.zeros((B, T, nv))


def expected(name, kind, cases):
    """Residual [B, T+1, nr], then cost [B, T+1], Lx [B, T+1, nv] and Lqq [B, T+1, nv, nv] of the differential model (no dt)."""
    r, J = cases[f"{name}_r"], cases[f"{name}_J"]
    if kind == _abi.RES_FRAME_ROTATION:  # log3 is the angular half of log6, Jlog3 the bottom-right block of Jlog6 (bottom left: 0)
        r, J = r[..., 3:], J[..., 3:, :]
    n = r.shape[1]
    i = np.arange(n) % r.shape[-1]
    ri, Ji = r[:, np.arange(n), i], J[:, np.arange(n), i]
    return r, 0.5 * ri * ri, ri[..., None] * Ji, Ji[..., :, None] * Ji[..., None, :]


@pytest.mark.parametrize("kind", [_abi.RES_FRAME_PLACEMENT, _abi.RES_FRAME_ROTATION], ids=["placement", "rotation"])
@pytest.mark.parametrize("name", GEN.DEVICE_MODELS)
def test_checker_nodes_with_a_log_row(cases, name, kind):
    table, po, ref, xs, us = row_problem(name, kind, cases)
    nv, T = table.nv, po.horizon
    sl = _abi.tile_slices(nv)
    r, cost, Lx, Lqq = expected(name, kind, cases)
    o = Oracle(table, po, 1)
    failures = []
    for b in range(xs.shape[0]):
        for t in range(T + 1):
            term = t == T
            tile, _, res = o.node_calc_diff(term, 0.0 if term else DT, xs[b, t], None if term else us[b, t], ref[b, t])
            s = 1.0 if term else DT
            fr, fJ = cases[f"{name}_floor_r"][b, t], cases[f"{name}_floor_J"][b, t]
            what = f"{name} b {b} node {t} theta {cases['device_theta'][t]:.9g}"
            compare(tile[sl["cost"]][0], s * cost[b, t], fr, what + " cost", failures)
            compare(tile[sl["Lx"]][:nv], s * Lx[b, t], fr + fJ, what + " Lx", failures)
            assert np.abs(tile[sl["Lx"]][nv:]).max() <= 1e-14
            compare(tile[sl["Lxx"]].reshape(2 * nv, 2 * nv)[:nv, :nv], s * Lqq[b, t], fJ, what + " Lxx", failures)
    assert not failures, "\n" + "\n".join(failures)
