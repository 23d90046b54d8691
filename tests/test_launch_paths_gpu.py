"""Every launch path the AGX_* switches select (launch_paths.PATHS; read in agx_ocp_create, csrc/agimus_hip.hip), at small sizes,
against the CPU checker and against the default path of the same problem.

Most other GPU tests run at B <= 7 with nothing set: the folded hand-off, the two-level sweep, the polled counters, the fused
derivative pass and speculative gains.  bench.py runs B = 1024 (k_publish3, the one-wave k_riccati_mx_pair), the profiles and
`bench.py --full` run the split derivative pass, skip empty launches, or take the gains on exit.  `large_batch` is the product
path of a big batch reached with a checker-sized problem.

Each (path, problem) pair asserts
  1. against the checker (one checker per instance where the instances have their own inertials or world): iter, solved and
     flags equal (qp_iters too for the constrained problem); xs / us / K / kkt / cost within the tolerances of the existing
     test of the problem class (launch_paths.TOL_*, each names its test).  An instance for which the checker reports a
     breakdown (flags bit 0) would be compared in its status words only, as test_fuzz_gpu.py does -- none of the problems
     has one (checked on the CPU);
  2. against the default handle: fold_off, copy_handoff and no_empty (they change how counters reach the host) and k1_split and
     profile (the split launches run the node body of the fused one) bitwise in xs, us, K and every status word; the other
     paths with equal iter / qp_iters / solved / flags and xs 1e-9, us 1e-8, K 1e-8 (relative, max norm), the bounds
     test_two_level_sweep.py puts between two sweeps of one solve (K 1e-9 in
     test_hip_parity.test_mfma_layout_sweep_agrees_with_the_lane_grid_sweep is for one direction, not a whole solve);
  3. download_first(copy=True) is node 0 / node 1 of download(), bitwise (copy_handoff: its own d_first route).

The MPC-loop leg runs eight steps of the resident sine trajectory with tile carry on and noisy measurements from step 1
(test_tile_carry_gpu._noise, first = 2), every path but the ADMM ones against the default handle.

Every solve runs once (module caches); the figures are printed before they are asserted."""
import numpy as np
import pytest

import launch_paths as lp
from agimus_controller_amd import _abi, workloads
from agimus_controller_amd.factory import robot_tables as rt
from test_plant_inertials_gpu import PAYLOAD
from test_tile_carry_gpu import _noise

pytestmark = pytest.mark.gpu

INT_WORDS = ("iter", "qp_iters", "solved", "flags")
SWEEP_TOL = dict(xs=1e-9, us=1e-8, K=1e-8)  # test_two_level_sweep.py (see the module docstring)
_SOLVES, _MPC = {}, {}


def rel(a, b):
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))


# ---------------------------------------------------------------------------------------------------------------- runs
def _snapshot(h, res):
    xs, us, K, st = res
    us0, K0, x1, _ = h.download_first(copy=True)
    d_xs, d_us, d_K, _ = h.download()
    return dict(xs=xs, us=us, K=K, st=np.array(st), first=(us0, K0, x1), resident=(d_xs, d_us, d_K))


def solve(backend, path, name):
    """{"full": snapshot} (+ "one" for the constrained problem) of problem `name` on `path`; computed once, left unchanged."""
    if (path, name) not in _SOLVES:
        p = lp.problem(name)
        out = {}
        with lp.handle(backend, lp.PATHS[path], p.table, p.po, p.B) as h:
            if path == "profile":
                h.profile(True)
            p.prepare(h)
            if p.constrained:
                out["one"] = _snapshot(h, h.solve(p.x0, p.xs, p.us, 1))
                h.reset_duals()
            out["full"] = _snapshot(h, h.solve(p.x0, p.xs, p.us, p.iters))
        _SOLVES[(path, name)] = out
    return _SOLVES[(path, name)]


MPC_STEPS, MPC_ITERS = 8, 10


def _mpc_problem(name):
    """goal: Panda, T = 13, B = 9; inert: T = 10, B = 3 with the inertials of launch_paths' `inert`.  One dt (tiles are carried)."""
    table = rt.panda_table(0.1)
    tcp = table.frame_id("panda_hand_tcp")
    T, B = (13, 9) if name == "goal" else (10, 3)
    running, terminal = workloads.goal_reaching_rows(tcp)
    po = _abi.PackedOcp(7, [0.01] * T, running, terminal, termination_tolerance=1e-3, max_qp_iters=100)
    inertials = workloads.stack_inertials(workloads.plant_tables(table, B, seed=5, payload=PAYLOAD)) if name == "inert" else None
    return table, tcp, po, B, T, inertials


def mpc(backend, path, name, profiled=False):
    """(steps, full_passes): per step (xs, us, K, status, first) and, on a profiled handle, the profile's count of passes over all
    running nodes."""
    key = (path, name, profiled or path == "profile")
    if key not in _MPC:
        table, tcp, po, B, T, inertials = _mpc_problem(name)
        noise = _noise(B, MPC_STEPS, 7, seed=977 + B)
        steps = []
        with lp.handle(backend, lp.PATHS[path], table, po, B) as h:
            q0, amp, puls, scale, t0 = workloads.sine_batch_params(B, lower=table.lower_position_limit, upper=table.upper_position_limit)
            w = workloads.SINE_WEIGHTS
            h.sine_trajectory(MPC_STEPS + T + 4, 0.01, q0, amp, puls, scale, t0, w["w_q"], w["w_qdot"], w["w_effort"], w["w_pose"], tcp)
            if inertials is not None:
                h.set_model_inertials(*inertials)
            if key[2]:
                h.profile(True)
            for k in range(MPC_STEPS):
                first = 1
                if k > 0:
                    h.upload_x0(steps[-1][4][2] + noise[:, k])
                    first = 2
                h.mpc_step(k, MPC_ITERS, first=first)
                us0, K0, x1, _ = h.download_first(copy=True)
                xs, us, K, st = h.download()
                steps.append((xs, us, K, np.array(st), (us0, K0, x1)))
            passes = h.profile(False)[1][0] if key[2] else None
        _MPC[key] = (steps, passes)
    return _MPC[key]


# ---------------------------------------------------------------------------------------------------------- comparisons
def _bound(what, got, want, tol, failures):
    """One figure against its bound: a max-norm relative bound (float) or (rtol, atol) as numpy.testing.assert_allclose."""
    if tol is None:
        return
    if isinstance(tol, tuple):
        worst = float((np.abs(got - want) / (tol[1] + tol[0] * np.abs(want) + 1e-300)).max())
        print(f"    {what}: max |diff| {np.abs(got - want).max():.3e}, {worst:.3e} of the bound rtol {tol[0]:g} atol {tol[1]:g}")
        ok = np.all(np.abs(got - want) <= tol[1] + tol[0] * np.abs(want))
    else:
        print(f"    {what}: relative {rel(got, want):.3e}, bound {tol:g}")
        ok = rel(got, want) < tol
    if not ok:
        failures.append(what)


def assert_matches_checker(got, want, tol, words, label):
    xs_o, us_o, K_o, st_o = want
    print(f"  {label} against the checker: iter {got['st']['iter'].tolist()} / {st_o['iter'].tolist()}, flags {got['st']['flags'].tolist()} / {st_o['flags'].tolist()}")
    for word in words:
        assert np.array_equal(got["st"][word], st_o[word]), (label, word, got["st"][word], st_o[word])
    keep = (st_o["flags"] & 1) == 0  # a breakdown in the checker: status words only
    assert keep.sum() >= len(keep) - 1
    failures = []
    _bound("xs", got["xs"][keep], xs_o[keep], tol["xs"], failures)
    _bound("us", got["us"][keep], us_o[keep], tol["us"], failures)
    _bound("K", got["K"][keep], K_o[keep], tol["K"], failures)
    _bound("kkt", got["st"]["kkt"][keep], st_o["kkt"][keep], tol["kkt"], failures)
    _bound("cost", got["st"]["cost"][keep], st_o["cost"][keep], tol["cost"], failures)
    assert not failures, (label, failures)


def assert_same_solve(got, ref, bitwise, label):
    """(xs, us, K, status) of two handles: every status word and every bit equal, or the integer words and SWEEP_TOL."""
    bits = [np.array_equal(a, b) for a, b in zip(got[:3], ref[:3])]
    print(f"  {label} against the default handle: bitwise xs / us / K {bits}; relative "
          f"{rel(got[0], ref[0]):.3e} / {rel(got[1], ref[1]):.3e} / {rel(got[2], ref[2]):.3e}")
    for word in (got[3].dtype.names if bitwise else INT_WORDS):
        assert np.array_equal(got[3][word], ref[3][word], equal_nan=True), (label, word, got[3][word], ref[3][word])
    if bitwise:
        assert all(bits), (label, bits)
    else:
        assert rel(got[0], ref[0]) < SWEEP_TOL["xs"] and rel(got[1], ref[1]) < SWEEP_TOL["us"] and rel(got[2], ref[2]) < SWEEP_TOL["K"], label


def assert_first_is_node_zero(first, resident, label):
    (us0, K0, x1), (xs, us, K) = first, resident
    assert np.array_equal(us0, us[:, 0]) and np.array_equal(K0, K[:, 0]) and np.array_equal(x1, xs[:, 1]), label


# ---------------------------------------------------------------------------------------------------------------- tests
def test_the_goal_problem_reaches_what_it_is_there_for():
    """The checker's own status words on `goal` (seed and cap chosen on the CPU): more than one line-search round, instances
    that finish in different iterations (stale tiles, the exit fix-up of the gains), nobody stopped by the cap."""
    st = lp.checker("goal")["full"][3]
    print("iter", st["iter"].tolist(), "flags", st["flags"].tolist(), "solved", st["solved"].tolist())
    assert len(set(st["iter"])) >= 2
    assert np.any(st["flags"] & 4)
    assert np.all(st["solved"] == 1) and st["iter"].max() < lp.GOAL_CAP
    for name in lp.MATRIX["default"]:
        if lp.problem(name).quorum is None:
            assert not np.any(lp.checker(name)["full"][3]["flags"] & 1), name  # nobody is excused from the comparison


@pytest.mark.parametrize("path,name", [(path, name) for path, names in lp.MATRIX.items() for name in names])
def test_solve(hip_backend, path, name):
    p = lp.problem(name)
    got = solve(hip_backend, path, name)
    words = INT_WORDS if p.constrained else ("iter", "solved", "flags")
    if p.quorum is None:
        want = lp.checker(name)
        if p.constrained:
            assert_matches_checker(got["one"], want["one"], lp.TOL_CON_ONE, INT_WORDS, f"{path} {name}, one iteration")
        assert_matches_checker(got["full"], want["full"], p.tol, words, f"{path} {name}")
    else:
        # the checker has no quorum: the instances the batch policy did not cut ran the checker's iterations, somebody was cut
        st, st_o = got["full"]["st"], lp.checker("goal")["full"][3]
        print(f"  {path} {name}: iter {st['iter'].tolist()}, solved {st['solved'].tolist()}")
        done = st["solved"] == 1
        assert 0 < done.sum() < p.B and np.array_equal(st["iter"][done], st_o["iter"][done])
    if path != "default":
        ref = solve(hip_backend, "default", name)
        for leg in got:
            a, b = got[leg], ref[leg]
            assert_same_solve((a["xs"], a["us"], a["K"], a["st"]), (b["xs"], b["us"], b["K"], b["st"]), path in lp.BITWISE, f"{path} {name} {leg}")
    for leg, snap in got.items():
        assert_first_is_node_zero(snap["first"], snap["resident"], f"{path} {name} {leg}")
        for a, b in zip(snap["resident"], (snap["xs"], snap["us"], snap["K"])):
            assert np.array_equal(a, b)


@pytest.mark.parametrize("name", lp.MPC_PROBLEMS)
@pytest.mark.parametrize("path", lp.MPC_PATHS)
def test_mpc_loop(hip_backend, path, name):
    """Eight MPC steps, tile carry on, noisy measurements: status words equal at every step, bitwise or within SWEEP_TOL as in
    test_solve.  `profile` is compared with a default handle that is profiled too (the host then skips empty launches on both).
    fold_off, copy_handoff and no_empty deliver n_carriable, which decides whether the next step inherits tiles, over three
    routes (the last workgroup of k_sqp_head / k_sqp_accept, k_publish3, the memcpys): a profiled handle of each counts as many
    passes over all running nodes as a profiled default handle."""
    profiled = path == "profile"
    runs = [(mpc(hip_backend, path, name), mpc(hip_backend, "default", name, profiled), "")]
    if path in lp.MPC_CARRY_COUNT:
        runs.append((mpc(hip_backend, path, name, True), mpc(hip_backend, "default", name, True), " (profiled)"))
    for (got, passes), (ref, ref_passes), tag in runs:
        for k, (a, b) in enumerate(zip(got, ref)):
            assert_same_solve(a[:4], b[:4], path in lp.BITWISE, f"{path} {name}{tag} step {k}")
            assert_first_is_node_zero(a[4], a[:3], f"{path} {name}{tag} step {k}")
        if tag:
            print(f"  passes over all running nodes of {MPC_STEPS} steps: {passes}, default {ref_passes}")
            assert passes == ref_passes
    iters = np.concatenate([s[3]["iter"] for s in runs[0][1][0][1:]])
    assert iters.max() >= 2, "the noise does not make the steps iterate"


def test_the_default_mpc_loop_carries_tiles(hip_backend):
    """What the pass counts of test_mpc_loop are measured against.  The profile counts the first pass of a step that carries
    no tiles and the first trial pass of every step: 2 x 8 without the carry (the noise makes every step search), at most 1 + 8
    when the steps after the first inherit their tiles."""
    for name in lp.MPC_PROBLEMS:
        _, passes = mpc(hip_backend, "default", name, True)
        print(name, "passes over all running nodes:", passes)
        assert passes <= MPC_STEPS + 1
