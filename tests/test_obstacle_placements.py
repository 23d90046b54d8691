"""Per-instance obstacle placements: what needs no GPU -- the argument checking of HipOcp.set_obstacle_placements /
clear_obstacle_placements against a stub that records what would reach the C ABI, the ABI surface, and the two workload
helpers (`obstacle_placements`, `world_tables`)."""
import ctypes as C
import pathlib
import re

import numpy as np
import pytest

from agimus_controller_amd import backend, workloads
from agimus_controller_amd.factory import robot_tables as rt

ROOT = pathlib.Path(__file__).resolve().parents[1]
B = 4


class RecordingLib:
    """Stands in for the loaded library: keeps the arguments of every agx_ocp_set_obstacle_placements call (arrays copied out
    while the call runs, as the library reads them)."""

    def __init__(self):
        self.calls = []

    def agx_ocp_set_obstacle_placements(self, handle, n, frames, se3):
        n = n.value
        fr = None if frames is None else np.ctypeslib.as_array(C.cast(frames, C.POINTER(C.c_int32)), shape=(n,)).copy()
        pl = None if se3 is None else np.ctypeslib.as_array(C.cast(se3, C.POINTER(C.c_double)), shape=(B, n, 12)).copy()
        self.calls.append((handle, n, fr, pl))
        return 0


def _table():
    return rt.panda_collision_table(0.1, obstacle_xyz=(0.45, 0.1, 0.45), obstacle_radius=0.08, obstacle_length=0.3,
                                    obstacles=workloads.random_obstacles(3))


@pytest.fixture
def stub(monkeypatch):
    lib = RecordingLib()
    monkeypatch.setattr(backend, "lib", lambda: lib)
    h = object.__new__(backend.HipOcp)  # no device: only the fields the two methods read
    h._h, h.B, h.nv, h.table = C.c_void_p(1234), B, 7, _table()
    yield h, lib
    h._h = None  # nothing to destroy


def test_arrays_reach_the_abi_in_order_and_layout(stub):
    h, lib = stub
    t = h.table
    frames = [t.frame_id("ob1"), t.frame_id("obstacle")]
    se3 = workloads.obstacle_placements(t, frames, B, seed=3)
    h.set_obstacle_placements(frames, se3)
    (handle, n, fr, pl), = lib.calls
    assert handle is h._h and n == 2
    np.testing.assert_array_equal(fr, frames)
    np.testing.assert_array_equal(pl, se3)
    # integer and non-contiguous inputs are converted
    ints = np.ones((B, 2, 12), dtype=int)
    h.set_obstacle_placements(np.array(frames, dtype=np.int64), ints)
    np.testing.assert_array_equal(lib.calls[1][3], np.ones((B, 2, 12)))
    h.set_obstacle_placements(frames, se3[:, :, ::-1][:, :, ::-1])
    np.testing.assert_array_equal(lib.calls[2][3], se3)
    h.set_obstacle_placements(frames[::-1], np.asfortranarray(se3[:, ::-1]))
    np.testing.assert_array_equal(lib.calls[3][2], frames[::-1])
    np.testing.assert_array_equal(lib.calls[3][3], se3[:, ::-1])


def test_names_resolve_to_ids(stub):
    h, lib = stub
    t = h.table
    se3 = workloads.obstacle_placements(t, ["ob0", "obstacle", "ob2"], B, seed=1)
    h.set_obstacle_placements(["ob0", t.frame_id("obstacle"), "ob2"], se3)
    np.testing.assert_array_equal(lib.calls[0][2], [t.frame_id("ob0"), t.frame_id("obstacle"), t.frame_id("ob2")])
    with pytest.raises(ValueError):
        h.set_obstacle_placements(["no_such_frame"], se3[:, :1])
    assert len(lib.calls) == 1


def test_clear_passes_zero_and_two_nulls(stub):
    h, lib = stub
    h.clear_obstacle_placements()
    assert lib.calls == [(h._h, 0, None, None)]


def test_wrong_shapes_are_refused_before_the_abi(stub):
    h, lib = stub
    frames = ["ob0", "ob1"]
    se3 = workloads.obstacle_placements(h.table, frames, B, seed=2)
    for bad in (se3[:2], se3[:, :1], se3[..., :9], se3.reshape(B, 24), se3[0]):
        with pytest.raises(ValueError, match="se3"):
            h.set_obstacle_placements(frames, bad)
    # the matrix forms are named
    for bad in (se3.reshape(B, 2, 3, 4), np.zeros((B, 2, 4, 4))):
        with pytest.raises(ValueError, match="matrix form"):
            h.set_obstacle_placements(frames, bad)
    with pytest.raises(ValueError, match="frames"):
        h.set_obstacle_placements([], np.zeros((B, 0, 12)))
    assert lib.calls == []


def test_a_refusal_of_the_library_is_raised(stub):
    h, lib = stub
    lib.agx_ocp_set_obstacle_placements = lambda *a: -1
    lib.agx_last_error = lambda: b"agx_ocp_set_obstacle_placements: frame listed twice (entry 1, frame 20)"
    with pytest.raises(backend.HipError, match="listed twice"):
        h.set_obstacle_placements(["ob0", "ob0"], np.zeros((B, 2, 12)))


def test_header_and_symbol_list_declare_the_entry_point():
    hdr = (ROOT / "include" / "agimus_hip.h").read_text()
    m = re.search(r"/\*((?:(?!\*/).)*)\*/\s*int\s+agx_ocp_set_obstacle_placements\s*\(\s*agx_ocp\s*\*\s*\w+\s*,\s*int\s+\w+\s*,\s*const\s+int32_t\s*\*\s*\w+\s*,"
                  r"\s*const\s+double\s*\*\s*\w+\s*\)\s*;", hdr, re.S)
    assert m, "the header does not declare agx_ocp_set_obstacle_placements"
    comment = " ".join(m.group(1).replace("*", " ").split())
    assert "at most 7 joints after padding" in comment  # the scope is part of the contract
    assert "not checked for orthonormality" in comment
    for stays in ("agx_model_frame_placement", "agx_model_frame_jacobian", "trajectory generators"):
        assert stays in comment
    assert "agx_ocp_set_obstacle_placements" in backend.EXPORTED_SYMBOLS
    for method in ("set_obstacle_placements", "clear_obstacle_placements"):
        assert callable(getattr(backend.HipOcp, method))


def test_obstacle_placements_are_seeded_bounded_and_keep_instance_zero():
    t = _table()
    frames = ["obstacle", "ob2"]
    a = workloads.obstacle_placements(t, frames, 5, seed=7, max_shift=0.1, max_angle=0.5)
    b = workloads.obstacle_placements(t, [t.frame_id(f) for f in frames], 5, seed=7, max_shift=0.1, max_angle=0.5)
    np.testing.assert_array_equal(a, b)
    assert a.shape == (5, 2, 12)
    assert not np.array_equal(a, workloads.obstacle_placements(t, frames, 5, seed=8))
    base = np.asarray(t.frame_placement).reshape(-1, 12)[[t.frame_id(f) for f in frames]]
    np.testing.assert_array_equal(a[0], base)
    for i in range(1, 5):
        for s in range(2):
            assert 0.0 < np.linalg.norm(a[i, s, 9:] - base[s, 9:]) <= 0.1 + 1e-15
            R = a[i, s, :9].reshape(3, 3)
            np.testing.assert_allclose(R @ R.T, np.eye(3), atol=1e-14)
            Rrel = R @ base[s, :9].reshape(3, 3).T
            angle = np.arccos(np.clip((np.trace(Rrel) - 1.0) / 2.0, -1.0, 1.0))
            assert 0.0 < angle <= 0.5 + 1e-12
    assert len({a[i].tobytes() for i in range(5)}) == 5


def test_world_tables_replace_the_listed_frames_only():
    t = _table()
    frames = ["ob1", "obstacle"]
    se3 = workloads.obstacle_placements(t, frames, 3, seed=5)
    tables = workloads.world_tables(t, frames, se3)
    again = workloads.world_tables(t, frames, se3)
    assert len(tables) == 3
    ids = [t.frame_id(f) for f in frames]
    rest = [f for f in range(len(t.frame_names)) if f not in ids]
    orig = np.asarray(t.frame_placement).reshape(-1, 12)
    for i, (w, w2) in enumerate(zip(tables, again)):
        fp = np.asarray(w.frame_placement)
        assert fp.shape == orig.shape and fp.dtype == orig.dtype
        np.testing.assert_array_equal(fp, np.asarray(w2.frame_placement))
        np.testing.assert_array_equal(fp[ids], se3[i])
        assert fp[rest].tobytes() == orig[rest].tobytes()  # bit-identical
        assert w.frame_names == t.frame_names and w.mass is t.mass
    np.testing.assert_array_equal(np.asarray(tables[0].frame_placement), orig)  # instance 0 is the table's own world
    assert np.asarray(t.frame_placement).reshape(-1, 12).tobytes() == orig.tobytes()  # the input is left alone
