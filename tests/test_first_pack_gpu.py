"""First-node results packed where instances finish (k_sqp_head, DESIGN.md section 4 "First-node record").

An instance that converges at the head of an SQP iteration whose gains sweep rode along writes its record
[us0 | K0 | x1 | status] into the mapped block itself; when every instance of a solve did, download_first hands the block out
without a launch.  Every other solve is packed by k_pack_first as before.  Whichever way a call is served, it must return what
the independent path download() (agx_ocp_download: us[:, 0], K[:, 0], xs[:, 1], status) returns, bit for bit."""

import numpy as np
import pytest

import launch_paths as lp
from agimus_controller_amd import _abi, workloads
from agimus_controller_amd.factory import robot_tables as rt

pytestmark = pytest.mark.gpu

MPC_STEPS, MPC_ITERS = 8, 10
# the large-batch hand-off with the host asking after the head before it queues a trial round: no early hand-off, same kernels
LARGE_BATCH_ASKING = {**lp.LARGE_BATCH, "AGX_NO_EMPTY_LAUNCHES": "1"}

WORDS = ("kkt", "cost", "merit", "gap_norm", "iter", "qp_iters", "solved", "flags")


def _bits(a):
    return np.ascontiguousarray(a).tobytes()


def check_first(h, label):
    """download_first(copy=True) against download(); returns (status of download(), the first-node arrays, 'in_solve' / 'launch')."""
    before = h.first_pack_counts()
    us0, K0, x1, st1 = h.download_first(copy=True)
    after = h.first_pack_counts()
    served = (after[0] - before[0], after[1] - before[1])
    assert served in ((1, 0), (0, 1)), f"{label}: one call, counted {served}"
    xs, us, K, st = h.download()
    assert _bits(us0) == _bits(us[:, 0]), f"{label}: us0"
    assert _bits(K0) == _bits(K[:, 0]), f"{label}: K0"
    assert _bits(x1) == _bits(xs[:, 1]), f"{label}: x1"
    for w in WORDS:
        assert st1[w].dtype == st[w].dtype and _bits(st1[w]) == _bits(st[w]), f"{label}: status word {w}: {st1[w]} / {st[w]}"
    return np.array(st), (us0, K0, x1, np.array(st1)), "in_solve" if served == (1, 0) else "launch"


def all_converged_in_a_paired_iteration(st):
    return bool(np.all(st["solved"] == 1) and np.all(st["iter"] >= 1))


def same_first(a, b, label):
    for name, va, vb in zip(("us0", "K0", "x1"), a[:3], b[:3]):
        assert _bits(va) == _bits(vb), f"{label}: {name} differs between in-solve pack on and off"
    for w in WORDS:
        assert _bits(a[3][w]) == _bits(b[3][w]), f"{label}: status word {w} differs between in-solve pack on and off"


def solve_on_and_off(backend, path, table, po, B, prepare, x0, xs, us, iters, label, exact):
    """One solve on a handle with the in-solve pack (the default) and on one with set_first_pack(0).  `exact`: "in_solve" where the
    solve converged everywhere at iter >= 1, "launch", or None (either; the counts add up)."""
    got = {}
    for on in (1, 0):
        with lp.handle(backend, lp.PATHS[path], table, po, B) as h:
            if not on:
                h.set_first_pack(0)
            prepare(h)
            h.download_first()  # the block is allocated by the first request; the head packs into it from the next solve on
            assert h.first_pack_counts() == (0, 1), f"{label}: a handle that has not solved served {h.first_pack_counts()}"
            h.solve(x0, xs, us, iters)
            st, first, served = check_first(h, f"{label} pack={on}")
            if not on:
                assert served == "launch", f"{label}: set_first_pack(0) served {served}"
            elif exact == "in_solve":
                if all_converged_in_a_paired_iteration(st):
                    assert served == "in_solve", f"{label}: every instance solved with iter >= 1 ({st['iter']}), served by {served}"
            elif exact == "launch":
                assert served == "launch", f"{label}: served {served}"
            calls = h.first_pack_counts()
            assert sum(calls) == 2, f"{label}: {calls} after two calls"
            got[on] = (st, first, served)
    same_first(got[1][1], got[0][1], label)
    return got[1]


def _problem_args(name):
    p = lp.problem(name)
    return p.table, p.po, p.B, p.prepare, p.x0, p.xs, p.us, p.iters


@pytest.mark.parametrize("path", ["default", "large_batch"])
def test_full_solve(hip_backend, path):
    st, _, served = solve_on_and_off(hip_backend, path, *_problem_args("goal"), f"goal/{path}", "in_solve")
    # (test_launch_paths_gpu.test_the_goal_problem_reaches_what_it_is_there_for: the problem converges in several iterations)
    assert all_converged_in_a_paired_iteration(st) and served == "in_solve", f"goal/{path}: iter {st['iter']} solved {st['solved']}"


@pytest.mark.parametrize("path", ["default", "large_batch"])
@pytest.mark.parametrize("name", ["goal_cap1", "goal_cap2", "goal_quorum"])
def test_cap_and_quorum(hip_backend, path, name):
    """Ends at the iteration cap without / with a paired gains sweep, or with an instance cut: whichever way the call is served."""
    solve_on_and_off(hip_backend, path, *_problem_args(name), f"{name}/{path}", None)


@pytest.mark.parametrize("B,T", [(1, 13), (205, 5)])
def test_batch_sizes(hip_backend, B, T):
    """B = 205 is the smallest batch that gets the hand-off of large batches (k_publish3, the early hand-off after the head) by default."""
    table = rt.panda_table(0.1)
    tcp = table.frame_id("panda_hand_tcp")
    po, ref, x0, xs, us = workloads.random_goal_problem(table, T, 0.01, B, 17, frame=tcp)
    solve_on_and_off(hip_backend, "default", table, po, B, lambda h: h.set_refs(ref), x0, xs, us, 12, f"B={B}", "in_solve")


def _mpc_problem():
    """Panda, goal rows on the tool, T = 13, B = 9, one dt (tiles are carried); measurement noise N(0, 0.2^2) rad on q and
    N(0, 1) rad/s on v from step 1 on, so that every step takes several iterations."""
    table = rt.panda_table(0.1)
    tcp = table.frame_id("panda_hand_tcp")
    T, B = 13, 9
    running, terminal = workloads.goal_reaching_rows(tcp)
    po = _abi.PackedOcp(7, [0.01] * T, running, terminal, termination_tolerance=1e-3, max_qp_iters=100)
    rng = np.random.default_rng(986)
    noise = np.concatenate([rng.normal(0.0, 0.2, (B, MPC_STEPS, 7)), rng.normal(0.0, 1.0, (B, MPC_STEPS, 7))], axis=-1)
    return table, tcp, po, B, T, noise


def _mpc_loop(backend, env, on, profiled, label):
    """Per step (status, first-node arrays, how the call was served, inheritable instances as published); the full derivative
    passes a profiled handle counted; the solves that ended on the hand-off right behind the head."""
    table, tcp, po, B, T, noise = _mpc_problem()
    steps = []
    with lp.handle(backend, env, table, po, B) as h:
        if not on:
            h.set_first_pack(0)
        q0, amp, puls, scale, t0 = workloads.sine_batch_params(B, lower=table.lower_position_limit, upper=table.upper_position_limit)
        w = workloads.SINE_WEIGHTS
        h.sine_trajectory(MPC_STEPS + T + 4, 0.01, q0, amp, puls, scale, t0, w["w_q"], w["w_qdot"], w["w_effort"], w["w_pose"], tcp)
        if profiled:
            h.profile(True)
        h.download_first()  # allocates the block
        for k in range(MPC_STEPS):
            first = 1
            if k > 0:
                h.upload_x0(steps[-1][1][2] + noise[:, k])
                first = 2
            h.mpc_step(k, MPC_ITERS, first=first)
            carriable = h.handoff_counts()[1]
            st, fst, served = check_first(h, f"mpc/{label} pack={on} step {k}")
            if not on:
                assert served == "launch", f"mpc/{label} step {k}: set_first_pack(0) served {served}"
            elif all_converged_in_a_paired_iteration(st):
                assert served == "in_solve", f"mpc/{label} step {k}: every instance solved with iter >= 1, served by {served}"
            steps.append((st, fst, served, carriable))
        assert sum(h.first_pack_counts()) == MPC_STEPS + 1
        passes = h.profile(False)[1][0] if profiled else None
        early = h.handoff_counts()[0]
    return steps, passes, early


@pytest.mark.parametrize("path", ["default", "large_batch"])
def test_mpc_loop(hip_backend, path):
    """Eight steps of the resident sine trajectory, noisy measurements from step 1 (several iterations per step); carried steps
    counted as tests/test_launch_paths_gpu.py does, by the full derivative passes a profiled handle reports."""
    env = lp.PATHS[path]
    on, _, early = _mpc_loop(hip_backend, env, 1, False, path)
    off, _, _ = _mpc_loop(hip_backend, env, 0, False, path)
    for k, (a, b) in enumerate(zip(on, off)):
        same_first(a[1], b[1], f"mpc/{path} step {k}")
        assert a[3] == b[3], f"mpc/{path} step {k}: {a[3]} inheritable instances with the in-solve pack, {b[3]} without"
    _, passes_on, _ = _mpc_loop(hip_backend, env, 1, True, path)
    _, passes_off, _ = _mpc_loop(hip_backend, env, 0, True, path)
    assert passes_on == passes_off, f"mpc/{path}: {passes_on} full derivative passes with the in-solve pack, {passes_off} without"
    if path == "default":
        assert early == 0, "a batch of 9 gets its counters from the head itself: no hand-off kernel behind it"
        return
    # A profiled handle asks after every head and never takes the early hand-off.  Without the profile: a step whose instances
    # all converged ends at the head of iteration max(iter); when that is not iteration 0 the host must have left on the words
    # published behind that head, and they must carry the count of inheritable instances the trial round's words carry on a
    # handle that always waits for them.
    expected = sum(1 for st, _, _, _ in on if np.all(st["solved"] == 1) and st["iter"].max() >= 1)
    assert expected >= 1, "no step converged everywhere after iteration 0: the case checks nothing"
    assert early == expected, f"{early} solves left on the hand-off behind the head, {expected} ended at a head after iteration 0"
    asking, _, early_asking = _mpc_loop(hip_backend, LARGE_BATCH_ASKING, 1, False, "large_batch, host asks")
    assert early_asking == 0
    for k, (a, b) in enumerate(zip(on, asking)):
        same_first(a[1], b[1], f"mpc/early hand-off step {k}")
        assert a[3] == b[3], f"step {k}: early hand-off published {a[3]} inheritable instances, the waiting host read {b[3]}"


def test_freshness_and_repeated_call(hip_backend):
    table, po, B, prepare, x0, xs, us, iters = _problem_args("goal")
    with lp.handle(hip_backend, lp.PATHS["default"], table, po, B) as h:
        prepare(h)
        h.download_first()  # allocates the block
        h.solve(x0, xs, us, iters)
        _, a, _ = check_first(h, "first call")
        _, b, _ = check_first(h, "second call")  # no solve in between: the same values
        same_first(a, b, "repeated call")
        h.shift_warmstart()  # xs, us move: the block packed during the solve is stale
        _, c, served = check_first(h, "after shift_warmstart")
        assert served == "launch"
        assert _bits(c[2]) != _bits(a[2]), "the shift did not move xs[1]: the case checks nothing"
        # and a solve after that is served from the block again
        h.solve(x0, xs, us, iters)
        st, d, served = check_first(h, "second solve")
        same_first(a, d, "second solve")
        if all_converged_in_a_paired_iteration(st):
            assert served == "in_solve"
        assert sum(h.first_pack_counts()) == 5


def test_views_without_copy(hip_backend):
    """copy=False hands out views of the block the head packed into."""
    table, po, B, prepare, x0, xs, us, iters = _problem_args("goal")
    with lp.handle(hip_backend, lp.PATHS["default"], table, po, B) as h:
        prepare(h)
        h.download_first()  # the block exists from the first request on
        xs_r, us_r, K_r, st = h.solve(x0, xs, us, iters)
        us0, K0, x1, words = h.download_first(copy=False)
        assert _bits(us0) == _bits(us_r[:, 0]) and _bits(K0) == _bits(K_r[:, 0]) and _bits(x1) == _bits(xs_r[:, 1])
        for w in WORDS:
            assert np.array_equal(words[w], st[w].astype(np.float64), equal_nan=True), w


def test_padded_model(hip_backend):
    """Five joints at the 7-joint capacity: the host removes the pad joints from whichever block it got."""
    table = rt.chain_table(5, seed=25)
    po, ref, x0, xs, us = workloads.random_goal_problem(table, 6, 0.01, 3, 31, frame=len(table.frame_names) - 1)
    solve_on_and_off(hip_backend, "default", table, po, 3, lambda h: h.set_refs(ref), x0, xs, us, 12, "nv5", None)


@pytest.mark.parametrize("path,name", [("default", "nv9"), ("default", "con"), ("copy_handoff", "goal"), ("gains_on_exit", "goal")])
def test_paths_that_keep_the_pack_launch(hip_backend, path, name):
    """Gains on exit (large models, AGX_SPECULATE_GAINS=0), constrained problems, no mapped block (AGX_HOST_POLL=0)."""
    solve_on_and_off(hip_backend, path, *_problem_args(name), f"{name}/{path}", "launch")
