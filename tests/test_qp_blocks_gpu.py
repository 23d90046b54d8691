"""Every block of the QP tile and the aux tile that the PRODUCTION derivative pass writes (launch_calc_qp -> launch_k1: the eight-lane
k_calc_qp_lj / k_calc_qp_lj_all, the one-lane k_calc_qp, k_calc_qp_wg<16|30|32> with k_cost_pairs and k_general_rows_wg behind
them) against the blocks rebuilt from the checker's canonical tile (tests/qp_blocks.py), once per launch path.  h.calc_diff() runs
other kernels (k_calc_diff), and direction() / solve() put a Riccati sweep between these blocks and what they assert.

Bound per block, running and terminal nodes apart: |got - want| <= tol x max |want| + 1e-14 + 8 x floor, with tol the value the
suite holds k_calc_diff to for the same row kinds (qp_blocks.QUAD / EXP / COLL / GEN) and floor the disagreement of the two routes
of the reference (tests/test_qp_blocks.py).  No block is left out; nothing is fitted to what the kernels return."""
import ctypes as C

import numpy as np
import pytest

import launch_paths
import qp_blocks as qb

pytestmark = pytest.mark.gpu

ZERO_AT_TERMINAL = ("Hqw", "Hvw", "Hww", "gw", "f", "M", "tq", "tv", "Luu", "Lu")  # calc_qp_term_body writes 0.0 into each


def _tiles(hip_backend, c, env=None):
    """h.qp_tiles() of the case on a handle created under its switches (plus env), as one dict, and the raw arrays."""
    with launch_paths.handle(hip_backend, dict(c.env, **(env or {})), c.table, c.po, c.B) as h:
        c.prepare(h)
        q, a = h.qp_tiles()
        got = {k: v.copy() for k, v in dict(q, **a).items()}
        qs, as_ = C.c_int(0), C.c_int(0)
        lib = hip_backend.lib()
        assert lib.agx_ocp_qp_tiles(h._h, None, None, C.byref(qs), C.byref(as_)) == 0
        qt, aux = np.empty((c.B, c.po.horizon + 1, qs.value)), np.empty((c.B, c.po.horizon + 1, as_.value))
        assert lib.agx_ocp_qp_tiles(h._h, qt.ctypes.data_as(C.c_void_p), aux.ctypes.data_as(C.c_void_p), C.byref(qs), C.byref(as_)) == 0
        flags = dict(general=bool(h.general_rows), wide=bool(h.cost_wide))
    return got, qt, aux, flags


def _pad_cross_terms(c, qt, aux):
    """DESIGN.md, "Model sizes at run time": every cross term between a pad joint and a real one is an exact zero -- in every
    NV x NV block of both tiles (raw arrays of agx_ocp_qp_tiles, rows of LD doubles)."""
    nv = c.nv
    ld = 8 if nv <= 7 else 32
    NV = (qt.shape[-1] - 5 * ld - 8) // (6 * ld)
    assert NV > nv and qt.shape[-1] == 6 * NV * ld + 5 * ld + 8 and aux.shape[-1] == 4 * NV * ld + 3 * ld, (nv, NV, qt.shape, aux.shape)
    for arr, names in ((qt, ("Hqq", "Hqv", "Hvv", "Hqw", "Hvw", "Hww")), (aux, ("M", "tq", "tv", "Lqq"))):
        for k, name in enumerate(names):
            blk = arr[..., k * NV * ld:(k + 1) * NV * ld].reshape(arr.shape[:-1] + (NV, ld))
            assert not blk[..., :nv, nv:NV].any(), (name, "real row, pad column")
            assert not blk[..., nv:NV, :nv].any(), (name, "pad row, real column")
            assert np.isfinite(blk).all(), name


@pytest.mark.parametrize("name", qb.CASES)
def test_production_tiles_against_the_reference(hip_backend, name):
    c = qb.case(name)
    want, floor, _ = qb.reference(name)
    got, qt, aux, flags = _tiles(hip_backend, c)
    assert flags["general"] == c.general and flags["wide"] == (name == "wide12")
    failures = []
    qb.compare_blocks(got, want, floor, c.tol, f"{c.path} / {name}", failures)
    for k in ZERO_AT_TERMINAL:
        assert not got[k][:, -1].any(), (k, "terminal node")
    if c.padded:
        _pad_cross_terms(c, qt, aux)
    assert not failures, "\n" + "\n".join(failures)


def test_eight_lane_split_launches_are_the_fused_kernel_bit_for_bit(hip_backend):
    """AGX_K1_FUSED=0 (k_calc_qp_lj per node type) against the default k_calc_qp_lj_all: the same node body, the same bits, in the
    raw arrays of both tiles; and therefore the same distance to the reference."""
    name, env = qb.SPLIT
    c = qb.case(name)
    want, floor, _ = qb.reference(name)
    fused, qt0, aux0, _ = _tiles(hip_backend, c)
    split, qt1, aux1, _ = _tiles(hip_backend, c, env)
    np.testing.assert_array_equal(qt1, qt0)
    np.testing.assert_array_equal(aux1, aux0)
    failures = []
    qb.compare_blocks(split, want, floor, c.tol, f"eight-lane split / {name}", failures)
    assert not failures, "\n" + "\n".join(failures)
