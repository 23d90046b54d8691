"""Shared by test_launch_paths_gpu.py and test_launch_switches.py: the launch paths (sets of AGX_* switches read by agx_ocp_create,
csrc/agimus_hip.hip), the small problems they are run on, and which path meets which problem.  Nothing here touches the GPU."""
import contextlib
import dataclasses
import functools
import os

import numpy as np

import test_many_collision_costs as mcc
from agimus_controller_amd import _abi, workloads
from agimus_controller_amd.factory import robot_tables as rt
from oracle.oracle import Oracle
from test_model_inertials_gpu import _collision_problem, checker_solves
from test_model_sizes import _model
from test_plant_inertials_gpu import PAYLOAD

# --------------------------------------------------------------------------------------------------------------- paths
# What a batch of more than 204 instances gets by default (bench.py runs B = 1024): k_publish3 hands the counters to the host,
# one wave per instance walks the horizon (k_riccati_mx_pair), no two-level sweep.
LARGE_BATCH = {"AGX_FOLD_PUBLISH": "0", "AGX_MX2_SEGMENTS": "0"}

PATHS = {
    "default": {},
    "large_batch": LARGE_BATCH,
    "fold_off": {"AGX_FOLD_PUBLISH": "0"},
    "copy_handoff": {"AGX_HOST_POLL": "0"},
    "no_empty": {"AGX_NO_EMPTY_LAUNCHES": "1", "AGX_FOLD_PUBLISH": "0"},
    "gains_on_exit": {"AGX_SPECULATE_GAINS": "0"},
    "k1_split": {"AGX_K1_FUSED": "0"},
    "profile": {},  # no switch: h.profile(True) before the solve
    "k1_one_lane": {"AGX_K1_LANES": "0"},
    "lane_grid": {"AGX_RICCATI_MX": "0"},
    "admm_one_wave": {"AGX_ADMM_SEGMENTS": "0"},
    "con_one_lane": {"AGX_CON_LANES": "0"},
    "admm_loop_0": {"AGX_ADMM_LOOP": "0", **LARGE_BATCH},
    "admm_loop_2": {"AGX_ADMM_LOOP": "2", **LARGE_BATCH},
}

GOAL = ["goal", "goal_cap1", "goal_cap2"]
NV7 = GOAL + ["coll_wq", "coll_qe", "wide12", "con", "inert", "obs", "obs_inert"]
K1_TABLES = ["goal", "coll_wq", "wide12", "inert", "obs", "obs_inert"]

# path -> problems it is compared on (with the checker and with the default handle); "goal_quorum" has no checker.
# large_batch on nv9 would set AGX_FOLD_PUBLISH alone (AGX_MX2_SEGMENTS is read for nv <= 7 only): that is fold_off on nv9.
MATRIX = {
    "default": NV7 + ["nv9", "goal_quorum"],
    "large_batch": NV7 + ["goal_quorum"],
    "fold_off": ["goal", "con", "nv9"],
    "copy_handoff": ["goal", "coll_qe", "con", "nv9"],
    "no_empty": ["goal", "nv9"],
    "gains_on_exit": GOAL + ["goal_quorum", "coll_qe", "inert"],
    "k1_split": K1_TABLES,
    "profile": K1_TABLES,
    "k1_one_lane": ["goal", "coll_wq", "inert", "obs"],
    "lane_grid": GOAL,
    "admm_one_wave": ["con"],
    "con_one_lane": ["con"],
    "admm_loop_0": ["con"],
    "admm_loop_2": ["con"],
}

# paths that change only how counters reach the host, or how the node body of the derivative pass is split over launches:
# bitwise the default handle in xs, us and K
BITWISE = ("fold_off", "copy_handoff", "no_empty", "k1_split", "profile")
# the MPC-loop leg: every path but the ADMM ones
MPC_PATHS = [p for p in PATHS if p not in ("default", "admm_one_wave", "con_one_lane", "admm_loop_0", "admm_loop_2")]
MPC_PROBLEMS = ["goal", "inert"]
# carry engaged equally (count of full derivative passes of a profiled handle) on the hand-offs that deliver n_carriable differently
MPC_CARRY_COUNT = ("fold_off", "copy_handoff", "no_empty")

# Switches that no path above sets, and the test file that runs each of them against the checker or the default path.
COVERED_ELSEWHERE = {
    "AGX_TILE_CARRY": "tests/test_tile_carry_gpu.py",           # carry on against carry off, bitwise, every test of the file
    "AGX_NODE_KKT_WIDE": "tests/test_node_passes_gpu.py",       # k_node_kkt against k_node_kkt_ahead
    "AGX_GAINS_MFMA": "tests/test_big_model.py",                # nv = 30 gains with and without the MFMA GEMM
    "AGX_CON_WIDE": "tests/test_many_collision_pairs.py",       # fixed against wide constraint layout
    "AGX_COST_WIDE": "tests/test_many_collision_costs.py",      # row table against wide cost path
    "AGX_ADMM_PREFACTOR": "tests/test_constraints.py",          # test_hip_lqr_pass_next_to_the_factorisation_is_the_same_solve
}


@contextlib.contextmanager
def handle(backend, env, table, po, B):
    """A handle created under the switches `env` (they are read in agx_ocp_create); the environment is put back at once."""
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        h = backend.HipOcp(table, po, B)
    finally:
        for k, v in old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v
    try:
        yield h
    finally:
        h.close()


# ------------------------------------------------------------------------------------------------------------ problems
# Tolerances against the checker, each the one of the existing test of the problem class (None: that test does not compare it).
# "rel": max-norm relative bounds; "allclose": (rtol, atol).
TOL_GOAL = dict(mode="rel", xs=1e-9, us=1e-9, K=1e-7, kkt=(1e-6, 1e-12), cost=(1e-10, 0.0))          # test_hip_parity.test_full_solve_matches_oracle
TOL_COLLISION = dict(mode="allclose", xs=(1e-6, 1e-7), us=(1e-6, 1e-6), K=(1e-5, 1e-5), kkt=None, cost=None)  # test_collision.test_hip_collision_tiles_and_solve_match_the_checker
TOL_WIDE = dict(mode="allclose", xs=(1e-8, 1e-10), us=(1e-8, 1e-8), K=1e-7, kkt=None, cost=None)      # test_many_collision_costs (full solves)
TOL_NV9 = dict(mode="allclose", xs=(1e-8, 1e-10), us=(1e-8, 1e-8), K=1e-7, kkt=(1e-5, 1e-10), cost=None)  # test_model_sizes.test_full_solve_and_shift
# test_constraints.test_hip_control_limits_match_the_checker: one SQP iteration tightly, then the full solve from fresh multipliers
TOL_CON_ONE = dict(mode="allclose", xs=(1e-8, 1e-9), us=(1e-7, 1e-7), K=(1e-6, 1e-6), kkt=(1e-6, 1e-9), cost=None)
TOL_CON_FULL = dict(mode="allclose", xs=(1e-6, 1e-6), us=(1e-5, 1e-5), K=None, kkt=None, cost=None)

GOAL_SEED, GOAL_CAP = 6, 12  # chosen on the CPU with the checker: see _goal
CON_ITERS = 6               # test_constraints.test_hip_admm_iterations_in_one_launch_are_the_same_solve


@dataclasses.dataclass
class Problem:
    name: str
    table: object
    po: object
    ref: np.ndarray
    x0: np.ndarray
    xs: np.ndarray
    us: np.ndarray
    iters: int
    tol: dict
    tables: list = None       # one checker table per instance (per-instance inertials / worlds)
    inertials: tuple = None   # set_model_inertials arguments
    obstacles: tuple = None   # set_obstacle_placements arguments
    quorum: float = None
    constrained: bool = False

    @property
    def B(self):
        return self.x0.shape[0]

    def prepare(self, h):
        h.set_refs(self.ref)
        if self.inertials is not None:
            h.set_model_inertials(*self.inertials)
        if self.obstacles is not None:
            h.set_obstacle_placements(*self.obstacles)
        if self.quorum is not None:
            h.set_quorum(self.quorum, self.quorum)


def _goal(name, iters, quorum=None):
    """Panda, goal rows on the tool, mixed dt, B = 9 (the second 8-instance group of k_riccati_mx_pair holds one instance),
    T = 13 (117 running nodes: not a multiple of 8; three segments of the two-level sweep by default)."""
    table = rt.panda_table(0.1)
    po, ref, x0, xs, us = workloads.random_goal_problem(table, 13, 0.01, 9, GOAL_SEED, frame=table.frame_id("panda_hand_tcp"),
                                                        timesteps=[0.01] * 7 + [0.02] * 4 + [0.04] * 2)
    return Problem(name, table, po, ref, x0, xs, us, iters, TOL_GOAL, quorum=quorum)


def _collision(name, activation):
    table, po, ref, x0, xs, us = _collision_problem(activation, 3, 6)
    return Problem(name, table, po, ref, x0, xs, us, 8, TOL_COLLISION)


def _obs(name, with_inertials):
    """coll_wq with a world per instance (instance 0 nominal); the second variant as
    test_obstacle_placements_gpu.test_together_with_model_inertials: instance 1 payload and moved obstacle, instance 2 nominal
    world and perturbed inertials."""
    p = _collision(name, _abi.ACT_WEIGHTED_QUAD)
    frames = ["obstacle"]
    se3 = workloads.obstacle_placements(p.table, frames, p.B, 0, 0.1, 0.5)
    if with_inertials:
        se3[2] = se3[0]
    p.tables = workloads.world_tables(p.table, frames, se3)
    p.obstacles = (frames, se3)
    if with_inertials:
        models = workloads.plant_tables(p.table, p.B, seed=5, payload=PAYLOAD)
        p.tables = [dataclasses.replace(m, frame_placement=w.frame_placement) for m, w in zip(models, p.tables)]
        p.inertials = workloads.stack_inertials(models)
    return p


def _con():
    """Panda, torque limits (15 N m) + a state box + link-7 capsule / obstacle distance >= 0.05, max_qp_iters = 100, B = 4, T = 12:
    k_con_eval_lj, the segmented ADMM sweeps, the prefactor launch and k_admm_loop for the tail."""
    table = rt.panda_collision_table(0.1, obstacle_xyz=(0.45, 0.1, 0.45), obstacle_radius=0.08, obstacle_length=0.3)
    tcp = table.frame_id("panda_hand_tcp")
    T, B = 12, 4
    running, terminal = workloads.goal_reaching_rows(tcp)
    lim = _abi.ConstraintSpec(_abi.RES_CONTROL, lower=-np.full(7, 15.0), upper=np.full(7, 15.0), name="ulim")
    box = _abi.ConstraintSpec(_abi.RES_STATE, lower=-5.0, upper=5.0, name="box")
    col = _abi.ConstraintSpec(_abi.RES_COLLISION, lower=0.05, upper=np.inf, frame=table.frame_id("panda_link7_capsule_0"),
                              frame_b=table.frame_id("obstacle"), name="collision")
    po = _abi.PackedOcp(7, [0.01] * T, running, terminal, max_qp_iters=100, running_constraints=[lim, box, col], terminal_constraints=[box, col])
    _, ref, x0, xs, us = workloads.random_goal_problem(table, T, 0.01, B, 3, frame=tcp)
    return Problem("con", table, po, ref, x0, xs, us, CON_ITERS, TOL_CON_FULL, constrained=True)


def _inert():
    """The panda_case of test_model_inertials_gpu.py: nominal | 2 kg payload | +-10 %."""
    table = rt.panda_table(0.1)
    po, ref, x0, xs, us = workloads.random_goal_problem(table, 10, 0.01, 3, 41, frame=table.frame_id("panda_hand_tcp"),
                                                        timesteps=[0.01] * 6 + [0.02] * 2 + [0.04] * 2)
    tables = workloads.plant_tables(table, 3, seed=5, payload=PAYLOAD)
    return Problem("inert", table, po, ref, x0, xs, us, 20, TOL_GOAL, tables=tables, inertials=workloads.stack_inertials(tables))


def _wide12():
    table = mcc._chain()
    po, ref, x0, xs, us = mcc._problem(table, 12, T=6)
    return Problem("wide12", table, po, ref, x0, xs, us, 8, TOL_WIDE)


def _nv9():
    """The Panda with its finger joints (a chain of 9, run at the 16-joint capacity): the workgroup kernels behind the same host loop."""
    table = _model(9, "panda_fingers")
    po, ref, x0, xs, us = workloads.random_goal_problem(table, 8, 0.01, 3, 109, frame=len(table.frame_names) - 1, timesteps=[0.01] * 5 + [0.02] * 3)
    return Problem("nv9", table, po, ref, x0, xs, us, 8, TOL_NV9)


_BUILDERS = {
    "goal": lambda: _goal("goal", GOAL_CAP),
    "goal_cap1": lambda: _goal("goal_cap1", 1),  # exits through the cap without a paired gains sweep
    "goal_cap2": lambda: _goal("goal_cap2", 2),  # ... with one
    "goal_quorum": lambda: _goal("goal_quorum", GOAL_CAP, quorum=0.8),
    "coll_wq": lambda: _collision("coll_wq", _abi.ACT_WEIGHTED_QUAD),
    "coll_qe": lambda: _collision("coll_qe", _abi.ACT_QUAD_EXP),
    "wide12": _wide12,
    "con": _con,
    "inert": _inert,
    "obs": lambda: _obs("obs", False),
    "obs_inert": lambda: _obs("obs_inert", True),
    "nv9": _nv9,
}


@functools.lru_cache(maxsize=None)
def problem(name):
    return _BUILDERS[name]()


def _stack(per):
    """checker_solves' {b: (xs, us, K, status)} of one-instance solves as one batch."""
    order = sorted(per)
    return tuple(np.concatenate([per[b][i] for b in order]) for i in range(4))


@functools.lru_cache(maxsize=None)
def checker(name):
    """The checker's solve of a problem, computed once and left unchanged: {"full": (xs, us, K, status)} and for the constrained
    problem also {"one": ...}, the first SQP iteration alone (the full solve then starts from fresh multipliers)."""
    p = problem(name)
    assert p.quorum is None, "the checker has no quorum"
    out = {}
    if p.tables is not None:
        out["full"] = _stack(checker_solves(p.tables, p.po, p.ref, p.x0, p.xs, p.us, p.iters))
        return out
    o = Oracle(p.table, p.po, p.B)
    if p.constrained:
        out["one"] = o.solve(p.ref, None, p.x0, p.xs, p.us, 1, nthreads=4)
        o.reset_duals()
    out["full"] = o.solve(p.ref, None, p.x0, p.xs, p.us, p.iters, nthreads=4)
    return out
