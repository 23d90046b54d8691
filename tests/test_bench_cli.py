"""bench.py's command line and its --dump-outputs writer (host logic only: no device needed)."""

import sys

import numpy as np
import pytest

import bench


def _parse(monkeypatch, *argv):
    monkeypatch.setattr(sys, "argv", ["bench.py", *argv])
    return bench.parse()


def test_a_plain_run_leaves_the_extra_measurements_to_full(monkeypatch):
    args = _parse(monkeypatch, "--gpus", "1", "--steps", "7", "--warmup", "2")
    assert args.steps == 7 and args.warmup == 2
    assert not args.full and args.dump_outputs is None
    args = _parse(monkeypatch, "--full", "--dump-outputs", "out")
    assert args.full and args.dump_outputs == "out"
    with pytest.raises(SystemExit):
        _parse(monkeypatch, "--steps", "0")


def _step_result(B, nv, seed=0):
    rng = np.random.default_rng(seed)
    st = {name: rng.normal(size=B) for name in ("kkt", "cost", "merit", "gap_norm", "iter", "qp_iters", "solved", "flags")}
    return rng.normal(size=(B, nv)), rng.normal(size=(B, nv, 2 * nv)), rng.normal(size=(B, 2 * nv)), st


def test_dump_outputs_writes_what_the_step_returned(tmp_path):
    res = _step_result(16, 7)
    outs = bench.first_node_outputs(res)
    bench.dump_outputs(tmp_path, outs)
    names = {p.stem for p in tmp_path.glob("*.npy")}
    assert names == {"us0", "K0", "x1"} | {f"status_{k}" for k in res[3]}
    for name, want in (("us0", res[0]), ("K0", res[1]), ("x1", res[2]), ("status_iter", res[3]["iter"])):
        got = np.load(tmp_path / f"{name}.npy")
        assert got.dtype == np.float64
        np.testing.assert_array_equal(got, want)


def test_dump_outputs_samples_instances_above_the_limit(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_LIMIT", 200_000)
    outs = bench.first_node_outputs(_step_result(1000, 7))
    for d in (tmp_path / "a", tmp_path / "b"):
        bench.dump_outputs(d, outs)
        assert sum(p.stat().st_size for p in d.glob("*.npy")) <= bench.DUMP_LIMIT
    idx = np.load(tmp_path / "a" / "instance_index.npy")
    assert 0 < idx.size < 1000 and np.all(np.diff(idx) > 0)
    np.testing.assert_array_equal(np.load(tmp_path / "a" / "K0.npy"), outs["K0"][idx.astype(int)])
    for p in (tmp_path / "a").glob("*.npy"):  # the same sample every time
        np.testing.assert_array_equal(np.load(p), np.load(tmp_path / "b" / p.name))
