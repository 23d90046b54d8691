"""Expected QP / aux tile blocks of the production derivative pass (launch_calc_qp), rebuilt from a canonical tile.  No GPU.

The production kernels (k_calc_qp_lj*, k_calc_qp, k_calc_qp_wg + k_cost_pairs + k_general_rows_wg) write the acceleration-form QP
tile and the aux tile (csrc/agx_tiles.hpp: QT, AUX; csrc/agx_kernels.hpp above calc_qp_body).  With du = tau_x dx + M dw the node's
quadratic model in (dx, du) becomes one in (dx, dw) by a congruence:

    P = [[I, 0], [tau_x, M]],   H_qp = P' [[Lxx, Lxu], [Lxu', Luu + preg I]] P,   g_qp = P' [Lx; Lu],   preg = 1e-9

(agx_ocp_qp_tiles resets the solver state, so preg is reg_min).  The terminal node has H = Lxx, gx = Lx and nothing else; f and cost
are copied.  The aux tile holds M | tq | tv | Lqq | Lvv | Luu | Lu with Lvv and Luu as DIAGONALS (one line each): every row kind
has a diagonal Luu, and of Lvv the aux tile keeps the share of the rows with a diagonal Lvv -- the dense share of a FrameVelocity
row travels in the general blocks (csrc/agx_general_rows.hpp), so for such a problem the caller passes Lvv_diag, the diagonal of a
canonical tile evaluated with the FrameVelocity rows' item weights set to zero (`without_rows`).

The dynamics blocks come by two independent routes:
  A  from the canonical tile itself: M = dt (Fu_v)^-1 (float64 inverse + Newton steps in longdouble), tq = -M Fx_vq / dt,
     tv = -M (Fx_vv - I) / dt;
  B  from tests/joint_ref.py: M = crba(q), (tq, tv) = complex-step Jacobian of rnea(q, v, a) at a = forward_dynamics(q, v, u).
Their disagreement per block is the FLOOR of a case: what the reference itself is uncertain about.  All arithmetic on the tiles is
done in np.longdouble.

The second half of this file is the list of cases, one per production launch path, shared by tests/test_qp_blocks.py (the
reference against itself, CPU) and tests/test_qp_blocks_gpu.py (the kernels against the reference).
"""
import dataclasses
import functools

import numpy as np

import joint_ref as jr
from agimus_controller_amd import _abi, workloads
from agimus_controller_amd.factory import robot_tables as rt
from oracle.oracle import Oracle

LD = np.longdouble
PREG = 1e-9
QP_BLOCKS = ("Hqq", "Hqv", "Hvv", "Hqw", "Hvw", "Hww", "gx", "gw", "f", "cost")
AUX_BLOCKS = ("M", "tq", "tv", "Lqq", "Lvv", "Luu", "Lu")
BLOCKS = QP_BLOCKS + AUX_BLOCKS
FLOOR_BOUND = 1e-12  # condition on the reference: floor <= FLOOR_BOUND x the block's largest entry
TS5 = [0.01, 0.02, 0.01, 0.04, 0.01]
TS3 = [0.01, 0.02, 0.04]


def _T(a):
    return np.swapaxes(a, -1, -2)


def ext_inverse(A, steps=3):
    """Inverse of a stack of matrices to longdouble round-off: float64 inverse, then Newton steps X <- X + X (I - A X)."""
    A = np.asarray(A, dtype=LD)
    X = np.linalg.inv(A.astype(np.float64)).astype(LD)
    eye = np.eye(A.shape[-1], dtype=LD)
    for _ in range(steps):
        X = X + X @ (eye - A @ X)
    return X


def dynamics_from_tiles(tiles, dts, nv, dtype=LD):
    """Route A.  (M, tq, tv) [B][T][nv][nv] of the running nodes from Fx | Fu of canonical tiles [B][T + 1][tile]."""
    sl = _abi.tile_slices(nv)
    B, T = tiles.shape[0], tiles.shape[1] - 1
    z = np.asarray(tiles[:, :T], dtype=dtype)
    dt = np.asarray(dts, dtype=dtype)[None, :, None, None]
    Fx, Fu = z[..., sl["Fx"]].reshape(B, T, 2 * nv, 2 * nv), z[..., sl["Fu"]].reshape(B, T, 2 * nv, nv)
    A = Fu[..., nv:, :] / dt
    M = ext_inverse(A) if dtype is LD else np.linalg.inv(A)
    tq = -M @ (Fx[..., nv:, :nv] / dt)
    tv = -M @ ((Fx[..., nv:, nv:] - np.eye(nv, dtype=dtype)) / dt)
    return M, tq, tv


def dynamics_from_model(tables, xs, us):
    """Route B.  tables: one table, or one per instance.  M = crba, tau_x by complex steps of rnea at a = forward_dynamics."""
    B, T = us.shape[:2]
    if not isinstance(tables, (list, tuple)):
        tables = [tables] * B
    nv = tables[0].nv
    M, tq, tv = (np.zeros((B, T, nv, nv)) for _ in range(3))
    for b, t in enumerate(tables):
        x, u = xs[b, :T], us[b]
        q, v = x[:, :nv], x[:, nv:]
        a = jr.forward_dynamics(t, q, v, u)
        M[b] = jr.crba(t, q)
        J = jr.cjac(lambda z: jr.rnea(t, z[..., :nv], z[..., nv:], a[:, None, :]), x)  # the armature term M a has no x in it
        tq[b], tv[b] = J[..., :nv], J[..., nv:]
    return M, tq, tv


def expected_blocks(tiles, dts, nv, dyn=None, Lvv_diag=None, preg=PREG):
    """Every block of the QP tile and of the aux tile, [B][T + 1][...] in np.longdouble, from canonical tiles [B][T + 1][tile].
    dyn: (M, tq, tv) of the running nodes (default: route A).  Lvv_diag [B][T + 1][nv]: see the module docstring."""
    sl = _abi.tile_slices(nv)
    B, T = tiles.shape[0], tiles.shape[1] - 1
    nx = 2 * nv
    z = np.asarray(tiles, dtype=LD)
    M, tq, tv = (np.asarray(a, dtype=LD) for a in (dynamics_from_tiles(tiles, dts, nv) if dyn is None else dyn))
    Lxx = z[..., sl["Lxx"]].reshape(B, T + 1, nx, nx)
    Lxu = z[..., sl["Lxu"]].reshape(B, T + 1, nx, nv)
    Luu = z[..., sl["Luu"]].reshape(B, T + 1, nv, nv)
    Lx, Lu = z[..., sl["Lx"]], z[..., sl["Lu"]]
    out = {k: np.zeros((B, T + 1, nv, nv), dtype=LD) for k in ("Hqq", "Hqv", "Hvv", "Hqw", "Hvw", "Hww", "M", "tq", "tv")}
    # running nodes: the congruence
    P = np.zeros((B, T, 3 * nv, 3 * nv), dtype=LD)
    P[..., :nx, :nx] = np.eye(nx, dtype=LD)
    P[..., nx:, :nv], P[..., nx:, nv:nx], P[..., nx:, nx:] = tq, tv, M
    Hc = np.zeros((B, T, 3 * nv, 3 * nv), dtype=LD)
    Hc[..., :nx, :nx], Hc[..., :nx, nx:], Hc[..., nx:, :nx] = Lxx[:, :T], Lxu[:, :T], _T(Lxu[:, :T])
    Hc[..., nx:, nx:] = Luu[:, :T] + LD(preg) * np.eye(nv, dtype=LD)
    H = _T(P) @ Hc @ P
    g = (_T(P) @ np.concatenate([Lx[:, :T], Lu[:, :T]], -1)[..., None])[..., 0]
    q, v, w = slice(0, nv), slice(nv, nx), slice(nx, 3 * nv)
    for name, (r, c) in dict(Hqq=(q, q), Hqv=(q, v), Hvv=(v, v), Hqw=(q, w), Hvw=(v, w), Hww=(w, w)).items():
        out[name][:, :T] = H[..., r, c]
    out["M"][:, :T], out["tq"][:, :T], out["tv"][:, :T] = M, tq, tv
    out["gx"] = np.concatenate([g[..., :nx], Lx[:, T:]], 1)
    out["gw"] = np.concatenate([g[..., nx:], np.zeros((B, 1, nv), dtype=LD)], 1)
    # terminal node: H = Lxx, gx = Lx
    out["Hqq"][:, T], out["Hqv"][:, T], out["Hvv"][:, T] = Lxx[:, T, q, q], Lxx[:, T, q, v], Lxx[:, T, v, v]
    out["f"], out["cost"] = z[..., sl["f"]], z[..., sl["cost"]][..., 0]
    # aux tile
    out["Lqq"] = Lxx[..., q, q]
    out["Lvv"] = np.diagonal(Lxx[..., v, v], axis1=-2, axis2=-1) if Lvv_diag is None else np.asarray(Lvv_diag, dtype=LD)
    out["Luu"] = np.diagonal(Luu, axis1=-2, axis2=-1)
    out["Lu"] = Lu
    assert not (Luu - out["Luu"][..., None] * np.eye(nv, dtype=LD)).any(), "the aux tile holds Luu as a diagonal"
    return out


def lvv_diagonal(tiles, nv):
    sl = _abi.tile_slices(nv)
    Lxx = tiles[..., sl["Lxx"]].reshape(tiles.shape[:-1] + (2 * nv, 2 * nv))
    return np.diagonal(Lxx[..., nv:, nv:], axis1=-2, axis2=-1)


def without_rows(po, ref, kinds):
    """The reference tile with the item weights of the rows of the given kinds set to zero: those rows add nothing."""
    ref = ref.copy()
    for term, rows in ((False, po.running), (True, po.terminal)):
        for i, r in enumerate(rows):
            if r.kind in kinds:
                po.row_view(ref, term, i)[0][...] = 0.0
    return ref


def floors(a, b):
    """{block: max |a - b|} of two sets of expected blocks."""
    return {k: float(np.abs(a[k] - b[k]).max()) for k in a}


def tolerance(tol, scale, floor):
    """tol: what the project holds k_calc_diff to for the same row kinds; 1e-14 and the factor 8: tests/test_log_maps.py."""
    return tol * scale + 1e-14 + 8.0 * floor


def compare_blocks(got, want, floor, tol, what, failures):
    """Every block, running and terminal nodes apart (running tiles carry dt, the terminal tile does not, so each gets its own
    scale): |got - want| <= tolerance(tol, largest |want| of the block over those nodes, floor).  A block that is zero by
    construction (terminal M, tq, tv, Hqw, Hvw, Hww, gw, f, Luu, Lu) is thereby asserted to be below 1e-14 + 8 floor; the callers
    assert exact zeros next to it.  Returns the worst err / bound over the blocks and prints it with its block and node."""
    worst = (0.0, None, None)
    T = want["cost"].shape[1] - 1
    for name in BLOCKS:
        g, w = np.asarray(got[name], dtype=LD), want[name]
        assert g.shape == w.shape, (what, name, g.shape, w.shape)
        for part, nodes in (("running", slice(0, T)), ("terminal", slice(T, T + 1))):
            err = np.abs(g[:, nodes] - w[:, nodes])
            bound = tolerance(tol, float(np.abs(w[:, nodes]).max()), floor[name])
            node_err = err.reshape(err.shape[0], err.shape[1], -1).max(-1)
            b, t = np.unravel_index(np.argmax(node_err), node_err.shape)
            ratio = float(node_err[b, t]) / bound
            if ratio > worst[0]:
                worst = (ratio, name, (int(b), int(t) + nodes.start))
            if not ratio <= 1.0:
                failures.append(f"{what} {name} ({part}) node {(int(b), int(t) + nodes.start)}: err {float(node_err[b, t]):.3e} > {bound:.3e}")
    print(f"{what}: worst block {worst[1]} node {worst[2]}: err / bound = {worst[0]:.3e} (tol {tol:.0e})")
    return worst


# --------------------------------------------------------------------------------------------------------------- cases
@dataclasses.dataclass
class Case:
    name: str
    path: str            # row of the table in DESIGN.md ("Which test pins which derivative kernel")
    table: object
    po: object
    ref: np.ndarray
    xs: np.ndarray
    us: np.ndarray
    tol: float
    env: dict = dataclasses.field(default_factory=dict)
    tables: list = None      # one checker table per instance (per-instance inertials / worlds)
    inertials: tuple = None  # set_model_inertials arguments
    obstacles: tuple = None  # set_obstacle_placements arguments
    prismatic: bool = False  # canonical tiles from joint_ref.calc_diff (the checker is revolute only)
    general: bool = False    # has ControlGrav / FrameVelocity rows
    padded: bool = False     # nv below the capacity it runs at: the pad joints' cross terms are checked too

    @property
    def B(self):
        return self.xs.shape[0]

    @property
    def nv(self):
        return self.table.nv

    def prepare(self, h):
        h.set_refs(self.ref)
        if self.inertials is not None:
            h.set_model_inertials(*self.inertials)
        if self.obstacles is not None:
            h.set_obstacle_placements(*self.obstacles)
        h.upload_warmstart(self.xs, self.us)


# tol per row kinds: quadratic rows 1e-11 (test_hip_parity.py::test_derivative_tiles), vector Exp / QuadExp rows 1e-10
# (test_exp_activations.py), collision-pair cost rows 1e-10 (test_many_collision_costs.py::_assert_tiles, the tighter of the two
# calc_diff bounds the suite has for collision rows at the 7-joint capacity), general rows 1e-10 (test_general_rows.py,
# test_general_rows_large.py: TOL16).
QUAD, EXP, COLL, GEN = 1e-11, 1e-10, 1e-10, 1e-10


def _goal(name, path, table, seed, big=False, **kw):
    B, ts = (2, TS3) if big else (3, TS5)
    frame = table.frame_id("panda_hand_tcp") if "panda_hand_tcp" in table.frame_names else len(table.frame_names) - 1
    po, ref, x0, xs, us = workloads.random_goal_problem(table, len(ts), 0.01, B, seed, frame=frame, timesteps=ts)
    return Case(name, path, table, po, ref, xs, us, QUAD, **kw)


def _collision(name, activation):
    from test_model_inertials_gpu import _collision_problem

    table, po, ref, x0, xs, us = _collision_problem(activation, 3, 5)
    return Case(name, "eight-lane, collision rows", table, po, ref, xs, us, COLL)


def _launch_path_problem(name):
    import launch_paths

    p = launch_paths.problem(name)
    return Case("lane8_" + name, "eight-lane, per-instance sources", p.table, p.po, p.ref, p.xs, p.us, QUAD if name == "inert" else COLL,
                tables=p.tables, inertials=p.inertials, obstacles=p.obstacles)


def _exp(name, act):
    import test_exp_activations as ea

    table = rt.panda_table(0.1)
    po, ref, x0, xs, us = ea._problem(table, 5, 3, 19, act, ea.ALL)
    return Case(name, "one lane per node", table, po, ref, xs, us, EXP)


def _general7():
    from test_general_rows import general_problem

    table = rt.panda_table(0.1)
    po, ref, x0, xs, us = general_problem(table, 5, 3, seed=13, ref_frame=1)
    return Case("lane1_general", "one lane per node", table, po, ref, xs, us, GEN, general=True)


def _wide():
    import test_many_collision_costs as mcc

    table = mcc._chain()
    po, ref, x0, xs, us = mcc._problem(table, 12, T=6)
    return Case("wide12", "wide cost set", table, po, ref, xs, us, COLL, padded=True)


def _sized(nv, kind):
    from test_model_sizes import _model

    return _goal(f"wg_{kind}{nv}", "workgroup kernel", _model(nv, kind), 200 + nv, big=True, padded=nv not in (16, 30, 32))


def _dense30():
    from test_big_model import _dense_rows_problem

    table, po, ref, xs, us = _dense_rows_problem(rt.humanoid30_table(), 4, 2, seed=11)
    return Case("wg_humanoid30_dense_rows", "workgroup kernel", table, po, ref, xs, us, EXP)  # a QuadExp / Exp collision row among them


def _general9():
    import test_general_rows_large as grl

    table, po, ref, x0, xs, us = grl._problem("tree9", 3, 47, ref_frame=2)
    return Case("wg_tree9_general", "workgroup kernel", table, po, ref, xs, us, GEN, general=True, padded=True)


def _prismatic(name, big):
    table, tool, _, _ = jr.prismatic_models()[name]
    B, ts = (2, TS3) if big else (3, TS5)
    po, ref, x0, xs, us = workloads.random_goal_problem(table, len(ts), 0.01, B, 80 + table.nv, frame=tool, timesteps=ts)
    return Case("prismatic_" + name, "prismatic", table, po, ref, xs, us, QUAD, prismatic=True, padded=table.nv in (9,))


_BUILDERS = {
    "lane8_panda": lambda: _goal("lane8_panda", "eight-lane fused", rt.panda_table(0.1), 101),
    "lane8_chain5": lambda: _goal("lane8_chain5", "eight-lane fused", rt.chain_table(5), 102, padded=True),
    "lane8_chain3": lambda: _goal("lane8_chain3", "eight-lane fused", rt.chain_table(3), 103, padded=True),
    "lane8_coll_wq": lambda: _collision("lane8_coll_wq", _abi.ACT_WEIGHTED_QUAD),
    "lane8_coll_qe": lambda: _collision("lane8_coll_qe", _abi.ACT_QUAD_EXP),
    "lane8_inert": lambda: _launch_path_problem("inert"),
    "lane8_obs": lambda: _launch_path_problem("obs"),
    "lane8_obs_inert": lambda: _launch_path_problem("obs_inert"),
    "lane1_panda": lambda: _goal("lane1_panda", "one lane per node", rt.panda_table(0.1), 101, env={"AGX_K1_LANES": "0"}),
    "lane1_tree6": lambda: _goal("lane1_tree6", "one lane per node", rt.tree_table(6), 104),
    "lane1_exp": lambda: _exp("lane1_exp", _abi.ACT_EXP),
    "lane1_quad_exp": lambda: _exp("lane1_quad_exp", _abi.ACT_QUAD_EXP),
    "lane1_general": _general7,
    "wide12": _wide,
    "wg_panda_fingers9": lambda: _sized(9, "panda_fingers"),
    "wg_tree16": lambda: _sized(16, "tree"),
    "wg_tree24": lambda: _sized(24, "tree"),
    "wg_chain31": lambda: _sized(31, "chain"),
    "wg_humanoid30_dense_rows": _dense30,
    "wg_tree9_general": _general9,
    "prismatic_gantry7": lambda: _prismatic("gantry7", False),
    "prismatic_panda_gripper": lambda: _prismatic("panda_gripper", True),
}
CASES = list(_BUILDERS)
SPLIT = ("lane8_panda", {"AGX_K1_FUSED": "0"})  # the eight-lane split launches: the fused result bit for bit


@functools.lru_cache(maxsize=None)
def case(name):
    return _BUILDERS[name]()


def canonical_tiles(c, ref=None):
    """[B][T + 1][tile] of a case from the checker (per instance where the case has a table per instance) or, for a model with
    prismatic joints, from joint_ref.calc_diff."""
    ref = c.ref if ref is None else ref
    if c.prismatic:
        return jr.calc_diff(c.table, c.po, ref, c.xs, c.us)
    if c.tables is not None:
        return np.concatenate([Oracle(c.tables[b], c.po, 1).calc_diff(ref[b:b + 1], None, c.xs[b:b + 1], c.us[b:b + 1]) for b in range(c.B)])
    return Oracle(c.table, c.po, c.B).calc_diff(ref, None, c.xs, c.us)


@functools.lru_cache(maxsize=None)
def reference(name):
    """(want, floor, tiles) of a case, computed once and left unchanged: the expected blocks by route A, the per-block
    disagreement with route B, the canonical tiles."""
    c = case(name)
    tiles = canonical_tiles(c)
    lvv = None
    if c.general:
        lvv = lvv_diagonal(canonical_tiles(c, without_rows(c.po, c.ref, (_abi.RES_FRAME_VELOCITY,))), c.nv)
    want = expected_blocks(tiles, c.po.dt, c.nv, Lvv_diag=lvv)
    other = expected_blocks(tiles, c.po.dt, c.nv, dyn=dynamics_from_model(c.tables if c.tables is not None else c.table, c.xs, c.us), Lvv_diag=lvv)
    return want, floors(want, other), tiles
