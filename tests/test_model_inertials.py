"""Per-instance controller inertials: what needs no GPU -- the argument checking of HipOcp.set_model_inertials /
clear_model_inertials against a stub that records what would reach the C ABI, and the ABI surface."""
import ctypes as C
import pathlib
import re

import numpy as np
import pytest

from agimus_controller_amd import backend, workloads
from agimus_controller_amd.factory import robot_tables as rt

ROOT = pathlib.Path(__file__).resolve().parents[1]


class RecordingLib:
    """Stands in for the loaded library: keeps the arguments of every agx_ocp_set_model_inertials call."""

    def __init__(self):
        self.calls = []

    def agx_ocp_set_model_inertials(self, handle, mass, com, inertia, armature):
        self.calls.append((handle, mass, com, inertia, armature))
        return 0


@pytest.fixture
def stub(monkeypatch):
    lib = RecordingLib()
    monkeypatch.setattr(backend, "lib", lambda: lib)
    h = object.__new__(backend.HipOcp)  # no device: only the fields the two methods read
    h._h, h.B, h.nv = C.c_void_p(1234), 4, 7
    yield h, lib
    h._h = None  # nothing to destroy


def _as_array(ptr, shape):
    return np.ctypeslib.as_array(C.cast(ptr, C.POINTER(C.c_double)), shape=shape)


def test_arrays_reach_the_abi_in_order_and_layout(stub):
    h, lib = stub
    tables = workloads.plant_tables(rt.panda_table(0.1), 4, seed=3, payload=(2.0, (0.0, 0.0, 0.1)))
    mass, com, inertia, armature = workloads.stack_inertials(tables)
    h.set_model_inertials(mass, com, inertia.reshape(4, 7, 3, 3), armature)  # [B][nv][3][3] is accepted as [B][nv][9]
    (handle, m, c, i, a), = lib.calls
    assert handle is h._h
    np.testing.assert_array_equal(_as_array(m, (4, 7)), mass)
    np.testing.assert_array_equal(_as_array(c, (4, 7, 3)), com)
    np.testing.assert_array_equal(_as_array(i, (4, 7, 9)), inertia)
    np.testing.assert_array_equal(_as_array(a, (4, 7)), armature)
    # integer and non-contiguous inputs are converted, armature None is NULL
    h.set_model_inertials(np.ones((4, 7), dtype=int), com[:, :, ::-1][:, :, ::-1], inertia)
    _, m, c, i, a = lib.calls[1]
    assert a is None
    np.testing.assert_array_equal(_as_array(m, (4, 7)), np.ones((4, 7)))
    np.testing.assert_array_equal(_as_array(c, (4, 7, 3)), com)


def test_clear_passes_four_nulls(stub):
    h, lib = stub
    h.clear_model_inertials()
    assert lib.calls == [(h._h, None, None, None, None)]


def test_wrong_shapes_are_refused_before_the_abi(stub):
    h, lib = stub
    mass, com, inertia, armature = workloads.stack_inertials([rt.panda_table(0.1)] * 4)
    for name, args in (("mass", (mass[:2], com, inertia)), ("mass", (mass[:, :6], com, inertia)), ("com", (mass, com[..., :2], inertia)),
                       ("inertia", (mass, com, inertia[..., :6])), ("inertia", (mass, com, inertia.reshape(4, 7, 9, 1))),
                       ("armature", (mass, com, inertia, armature[:, :5]))):
        with pytest.raises(ValueError, match=name):
            h.set_model_inertials(*args)
    assert lib.calls == []


def test_a_refusal_of_the_library_is_raised(stub, monkeypatch):
    h, lib = stub
    lib.agx_ocp_set_model_inertials = lambda *a: -1
    lib.agx_last_error = lambda: b"agx_ocp_set_model_inertials: negative mass (instance 1, joint 3)"
    mass, com, inertia, _ = workloads.stack_inertials([rt.panda_table(0.1)] * 4)
    with pytest.raises(backend.HipError, match="negative mass"):
        h.set_model_inertials(mass, com, inertia)


def test_header_and_symbol_list_declare_the_entry_point():
    hdr = (ROOT / "include" / "agimus_hip.h").read_text()
    assert re.search(r"\bint\s+agx_ocp_set_model_inertials\s*\(\s*agx_ocp\s*\*", hdr)
    assert "agx_ocp_set_model_inertials" in backend.EXPORTED_SYMBOLS
    assert "at most 7 joints after padding" in hdr  # the scope is part of the contract
    for method in ("set_model_inertials", "clear_model_inertials"):
        assert callable(getattr(backend.HipOcp, method))
