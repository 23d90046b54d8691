"""The log maps of the HIP kernels against exact values: nodes whose frame sits at a rotation angle theta from the node's reference
placement, theta on the grid of tests/golden/make_log_map_fixture.py (0, every threshold of log3 / log6 / Jlog3 / Jlog6 from both
sides, up to pi - 1e-5), translations 0, 1e-3 and 0.5.  The fixture holds q, Mref and, by mpmath from those doubles, the residual
r = log6(Mref^-1 M(q)) and dr/dq (central differences in q: no Jacobian formula of the frame or of the log enters).  B = 2, T = 20.

One problem per launch path and row kind: a FramePlacement (log6, Jlog6) or a FrameRotation (log3, Jlog3) row with unit item
weight next to a Control row of weight zero, so Lu = 0 and the QP tile's gx is Lx.  The activation weights of node t are the unit
vector e_(t mod nr): cost = r_i^2 / 2, Lx = r_i J_i and the Gauss-Newton Lxx = J_i' J_i show single rows of Jlog.
  panda           eight-lane kernel         residuals, item_costs, calc_diff, qp_tiles
  tree6           one lane per node         the same reads
  panda_fingers   workgroup, capacity 16    item_costs, calc_diff, qp_tiles
Constraint rows: the library has no readback of g or its Jacobian and a constraint row has one reference for all nodes, so the
constraint evaluation of these rows is NOT checked here (it calls the same log6<JAC> / log3 / jlog3).

Tolerance, floor and the factor 8: tests/test_log_maps.py (1e-11 x the node's largest reference entry + 1e-14 + 8 x floor; the
largest floor of these nodes is 4.8e-14 for r and 2.7e-14 for dr/dq, at pi - 1e-2 - 1e-4).  No case is skipped."""
import numpy as np
import pytest

import test_log_maps as lm
from agimus_controller_amd import _abi

pytestmark = pytest.mark.gpu

KINDS = {"placement": _abi.RES_FRAME_PLACEMENT, "rotation": _abi.RES_FRAME_ROTATION}


@pytest.fixture(scope="module")
def cases():
    return dict(np.load(lm.GOLDEN / "log_map_cases.npz"))


def compare_nodes(got, want, floor, what, failures):
    """Per node (leading axes of floor): |got - want| <= tolerance(largest |want| of the node, floor of the node)."""
    assert got.shape == want.shape, (what, got.shape, want.shape)
    tail = tuple(range(floor.ndim, want.ndim))
    err = np.abs(got - want).max(tail) if tail else np.abs(got - want)
    scale = np.abs(want).max(tail) if tail else np.abs(want)
    tol = lm.tolerance(scale, floor)
    worst = np.unravel_index(np.argmax(err / tol), err.shape)
    print(f"{what}: worst node {worst}: err {err[worst]:.3e} tol {tol[worst]:.3e} (scale {scale[worst]:.3e}, floor {floor[worst]:.1e})")
    for idx in zip(*np.nonzero(~(err <= tol))):
        failures.append(f"{what} node {idx}: err {err[idx]:.3e} > {tol[idx]:.3e}")


@pytest.mark.parametrize("kind", list(KINDS))
@pytest.mark.parametrize("name", lm.GEN.DEVICE_MODELS)
def test_log_rows_against_exact_values(hip_backend, cases, name, kind):
    table, po, ref, xs, us = lm.row_problem(name, KINDS[kind], cases)
    B, T, nv = xs.shape[0], po.horizon, table.nv
    assert B <= 4 and T <= 31
    r, cost, Lx, Lqq = lm.expected(name, KINDS[kind], cases)
    fr, fJ = cases[f"{name}_floor_r"], cases[f"{name}_floor_J"]
    dt = np.concatenate([np.full(T, lm.DT), [1.0]])  # running nodes carry dt in the tiles, the terminal node does not
    h = hip_backend.HipOcp(table, po, B)
    h.set_refs(ref)
    h.upload_warmstart(xs, us)
    failures = []
    if name != "panda_fingers":
        compare_nodes(h.residuals(1), r[:, :T], fr[:, :T], "residuals", failures)
    it = h.item_costs()
    assert not it["cost_r"][:, :, 0].any() and not it["Lx_r"][:, :, 0].any() and not it["Lu_r"].any()
    compare_nodes(it["cost_r"][:, :, 1], cost[:, :T], fr[:, :T], "item cost, running", failures)
    compare_nodes(it["Lx_r"][:, :, 1, :nv], Lx[:, :T], (fr + fJ)[:, :T], "item Lx, running", failures)
    compare_nodes(it["cost_t"][:, 0], cost[:, T], fr[:, T], "item cost, terminal", failures)
    compare_nodes(it["Lx_t"][:, 0, :nv], Lx[:, T], (fr + fJ)[:, T], "item Lx, terminal", failures)
    assert not it["Lx_r"][..., nv:].any() and not it["Lx_t"][..., nv:].any()
    sl = _abi.tile_slices(nv)
    tiles = h.calc_diff()
    compare_nodes(tiles[..., sl["cost"]][..., 0], cost * dt, fr, "calc_diff cost", failures)
    compare_nodes(tiles[..., sl["Lx"]][..., :nv], Lx * dt[:, None], fr + fJ, "calc_diff Lx", failures)
    Lxx = tiles[..., sl["Lxx"]].reshape(B, T + 1, 2 * nv, 2 * nv)
    compare_nodes(Lxx[..., :nv, :nv], Lqq * dt[:, None, None], fJ, "calc_diff Lxx", failures)
    assert not tiles[..., sl["Lx"]][..., nv:].any() and not Lxx[..., nv:, :].any() and not Lxx[..., :, nv:].any()
    assert not tiles[..., sl["Lu"]].any()
    q, a = h.qp_tiles()
    compare_nodes(q["cost"], cost * dt, fr, "qp_tiles cost", failures)
    compare_nodes(q["gx"][..., :nv], Lx * dt[:, None], fr + fJ, "qp_tiles gx", failures)
    compare_nodes(a["Lqq"], Lqq * dt[:, None, None], fJ, "qp_tiles Lqq", failures)
    assert not q["gx"][..., nv:].any()
    h.close()
    assert not failures, "\n" + "\n".join(failures)
