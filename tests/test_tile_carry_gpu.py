"""Tile carry across MPC steps: a step that follows the previous one by one sample inherits the derivative
tiles of the old nodes 1 .. T-1 as its nodes 0 .. T-2 (a ring of tile slots) and evaluates nodes 0, T-1 and T only.  The carried
tiles are the same bits a full pass writes, so everything a solve hands out must be bitwise equal with AGX_TILE_CARRY=0 and 1
(the switch is read when a handle is created: both handles live in this process)."""

import os

import numpy as np
import pytest

from agimus_controller_amd import _abi, workloads
from agimus_controller_amd.factory import robot_tables as rt

pytestmark = pytest.mark.gpu

DT = 0.01
N_STEPS = 14  # >= 12, and more than T of the small-T cases: the ring wraps
SIGMA = 0.2   # bench.py --disturb-sigma: N(0, sigma^2) rad on q, N(0, (5 sigma)^2) rad/s on v


def _handle(backend, carry, table, po, B, n_points, frame, seed0=1234):
    old = os.environ.get("AGX_TILE_CARRY")
    os.environ["AGX_TILE_CARRY"] = "1" if carry else "0"
    try:
        h = backend.HipOcp(table, po, B)
    finally:
        if old is None:
            del os.environ["AGX_TILE_CARRY"]
        else:
            os.environ["AGX_TILE_CARRY"] = old
    nv = table.nv
    q0, amp, puls, scale, t0 = workloads.sine_batch_params(B, nv=nv, seed0=seed0, q0=(None if nv == 7 else np.zeros(nv)),
                                                           lower=table.lower_position_limit, upper=table.upper_position_limit)
    w = workloads.SINE_WEIGHTS
    h.sine_trajectory(n_points, DT, q0, amp, puls, scale, t0, w["w_q"], w["w_qdot"], w["w_effort"], w["w_pose"], frame)
    return h


def _panda(T, dts=None, constraints=()):
    table = rt.panda_table(0.1)
    tcp = table.frame_id("panda_hand_tcp")
    running, terminal = workloads.goal_reaching_rows(tcp)
    po = _abi.PackedOcp(7, list(dts) if dts is not None else [DT] * T, running, terminal, termination_tolerance=1e-3, max_qp_iters=100,
                        running_constraints=list(constraints))
    return table, tcp, po


def _snapshot(h):
    xs, us, K, st = h.download()
    return xs, us, K, np.array(st)


def _noise(B, n, nv, seed):
    rng = np.random.default_rng(seed)
    z = np.empty((B, n, 2 * nv))
    z[..., :nv] = rng.normal(0.0, SIGMA, (B, n, nv))
    z[..., nv:] = rng.normal(0.0, 5.0 * SIGMA, (B, n, nv))
    return z


def _run(backend, carry, table, po, B, frame, n_steps=N_STEPS, max_iter=10, noise=None, quorum=None, between=None):
    """n_steps consecutive MPC steps; `between(h, k)` runs before step k and returns the `first` argument of that step (or None)."""
    T = po.horizon
    h = _handle(backend, carry, table, po, B, n_steps + T + 4, frame)
    if quorum is not None:
        h.set_quorum(quorum, quorum)
    out = []
    for k in range(n_steps):
        first = 1 if k == 0 else 0
        if k > 0 and noise is not None:
            x1 = np.array(h.download_first(copy=True)[2])
            h.upload_x0(x1 + noise[:, k])
            first = 2
        if between is not None and k > 0:
            f = between(h, k)
            first = first if f is None else f
        h.mpc_step(k, max_iter, first=first)
        out.append(_snapshot(h))
    return h, out


def _assert_equal_runs(a, b):
    assert len(a) == len(b)
    for k, (ra, rb) in enumerate(zip(a, b)):
        for name, va, vb in zip(("xs", "us", "K"), ra[:3], rb[:3]):
            assert np.array_equal(va, vb), f"step {k}: {name} differs (max |diff| {np.abs(va - vb).max():.3e})"
        for field in ra[3].dtype.names:
            assert np.array_equal(ra[3][field], rb[3][field], equal_nan=True), f"step {k}: status word {field} differs"


def _both(backend, table, po, B, frame, **kw):
    h1, on = _run(backend, True, table, po, B, frame, **kw)
    h0, off = _run(backend, False, table, po, B, frame, **kw)
    _assert_equal_runs(on, off)
    return h1, h0, on


@pytest.mark.parametrize("T", [1, 2, 3, 37])
@pytest.mark.parametrize("B", [3, 256])
def test_prediction_loop(hip_backend, T, B):
    """x0 <- previous xs[1]; B = 3 runs the two-level sweeps, B = 256 the one-wave sweeps; T = 1, 2, 3: the ring wraps many times."""
    table, tcp, po = _panda(T)
    h1, h0, _ = _both(hip_backend, table, po, B, tcp)
    h1.close(); h0.close()


@pytest.mark.parametrize("B", [64, 256])
def test_noisy_measurements_backtrack(hip_backend, B):
    """x0 uploaded with noise every step: several SQP iterations, rejected step lengths (status flag bit 2 = a step length < 1 was tried).
    B = 64 runs the two-level sweeps, B = 256 the one-wave sweeps.  Batches of this size because a step length is rejected in
    about 2 % of the instance-steps under this noise (profiles/r03_bench_sine.json: 599 of 24 576): 13 noisy steps of 64
    instances hold ~ 20 of them, three instances ~ 1 (a seed can easily have none)."""
    T = 20
    table, tcp, po = _panda(T)
    noise = _noise(B, N_STEPS, 7, seed=977 + 1234)
    h1, h0, runs = _both(hip_backend, table, po, B, tcp, noise=noise)
    flags = np.concatenate([r[3]["flags"] for r in runs[1:]])
    iters = np.concatenate([r[3]["iter"] for r in runs[1:]])
    assert np.any(flags & 4), "no instance backtracked: the case does not exercise the line search"
    assert iters.max() >= 2
    h1.close(); h0.close()


def test_five_joints_padded_to_seven(hip_backend):
    table = rt.chain_table(5, seed=25)
    frame = len(table.frame_names) - 1
    T = 12
    running, terminal = workloads.goal_reaching_rows(frame)
    po = _abi.PackedOcp(5, [DT] * T, running, terminal, termination_tolerance=1e-3, max_qp_iters=100)
    h1, h0, _ = _both(hip_backend, table, po, 4, frame)
    h1.close(); h0.close()


@pytest.mark.parametrize("noisy", [False, True])
def test_one_iteration_per_step(hip_backend, noisy):
    """max_iter = 1: no instance converges, every step ends inside the iteration cap (tiles of the accepted trial are carried)."""
    T, B = 10, 5
    table, tcp, po = _panda(T)
    noise = _noise(B, N_STEPS, 7, seed=5) if noisy else None
    h1, h0, _ = _both(hip_backend, table, po, B, tcp, max_iter=1, noise=noise)
    h1.close(); h0.close()


def test_mixed_dt_switches_the_carry_off(hip_backend):
    T, B = 8, 4
    table, tcp, po = _panda(T, dts=[DT] * 5 + [2 * DT] * 3)
    h1, h0, _ = _both(hip_backend, table, po, B, tcp)
    h1.close(); h0.close()


@pytest.mark.parametrize("what", ["set_refs", "upload_xs", "first"])
def test_invalidation_then_resume(hip_backend, what):
    """Something that changes an input of the derivative pass between two steps: the next step runs the full pass, later ones carry again."""
    T, B = 6, 4
    table, tcp, po = _panda(T)
    rng = np.random.default_rng(3)
    bump = 1e-3 * rng.standard_normal((B, T + 1, 14))

    def between(h, k):
        if k not in (5, 9):
            return None
        if what == "set_refs":
            # a host tile replaces the window for one direct solve; the next mpc_step goes back to the resident trajectory
            ref = np.zeros((B, T + 1, h.stride))
            ref[..., 0] = 1.0
            h.set_refs(ref)
            return None
        if what == "upload_xs":
            xs, us, _, _ = h.download()
            h.upload_warmstart(xs + bump, us)
            return None
        return 1

    h1, h0, _ = _both(hip_backend, table, po, B, tcp, between=between)
    h1.close(); h0.close()


def test_quorum(hip_backend):
    """Quorum 0.9: the batch step ends with instances cut between iterations; those with stale tiles run the full pass."""
    T, B = 16, 20
    table, tcp, po = _panda(T)
    noise = _noise(B, N_STEPS, 7, seed=11)
    h1, h0, runs = _both(hip_backend, table, po, B, tcp, noise=noise, quorum=0.9)
    assert any(np.any(r[3]["solved"] == 0) for r in runs[1:]), "the quorum never cut an instance"
    h1.close(); h0.close()


def test_qp_tiles_after_a_wrapped_ring(hip_backend):
    """The debug reader returns the tiles in node order whatever the ring origin was."""
    T, B = 5, 3
    table, tcp, po = _panda(T)
    h1, h0, _ = _both(hip_backend, table, po, B, tcp, n_steps=T + 3)
    q1, a1 = h1.qp_tiles()
    q0, a0 = h0.qp_tiles()
    for k in q0:
        assert np.array_equal(q1[k], q0[k]), k
    for k in a0:
        assert np.array_equal(a1[k], a0[k]), k
    # and the loop goes on from there (the reader ended the carry)
    for h in (h1, h0):
        h.mpc_step(T + 3, 10, first=0)
    _assert_equal_runs([_snapshot(h1)], [_snapshot(h0)])
    h1.close(); h0.close()


def test_constrained_handle_is_untouched(hip_backend):
    """Constraint data is not carried: a constrained handle keeps the full pass (ring origin 0) under either switch value."""
    T, B = 10, 3
    lim = _abi.ConstraintSpec(_abi.RES_CONTROL, lower=-np.full(7, 40.0), upper=np.full(7, 40.0), name="ulim")
    table, tcp, po = _panda(T, constraints=[lim])
    h1, h0, _ = _both(hip_backend, table, po, B, tcp)
    q1, a1 = h1.qp_tiles()
    q0, a0 = h0.qp_tiles()
    for k in q0:
        assert np.array_equal(q1[k], q0[k]), k
    h1.close(); h0.close()
