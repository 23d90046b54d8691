"""Keeps the list of launch switches honest: every AGX_* variable the library reads is documented in the README switch table and
is either set by a path of test_launch_paths_gpu.py (launch_paths.PATHS / MATRIX) or named in launch_paths.COVERED_ELSEWHERE with
the test file that runs it.  A switch added without a test fails here."""
import pathlib
import re

import launch_paths as lp

ROOT = pathlib.Path(__file__).resolve().parents[1]


def _switches_read_by_the_library():
    names = set()
    for src in sorted((ROOT / "agimus_controller_amd" / "csrc").iterdir()):
        if src.suffix in (".hip", ".hpp", ".h", ".cpp"):
            names |= set(re.findall(r'getenv\(\s*"(AGX_[A-Z0-9_]+)"\s*\)', src.read_text()))
    return names


def _readme_switch_table():
    rows = set()
    for line in (ROOT / "README.md").read_text().splitlines():
        m = re.match(r"\|\s*`(AGX_[A-Z0-9_]+)", line)
        if m:
            rows.add(m.group(1))
    return rows


def test_the_library_reads_switches_at_all():
    names = _switches_read_by_the_library()
    assert {"AGX_K1_FUSED", "AGX_HOST_POLL", "AGX_FOLD_PUBLISH"} <= names and len(names) >= 17, names


def test_every_switch_has_a_readme_row():
    missing = _switches_read_by_the_library() - _readme_switch_table()
    assert not missing, f"README.md switch table lacks {sorted(missing)}"


def test_every_switch_is_run_by_a_test():
    set_by_a_path = set()
    for path, names in lp.MATRIX.items():
        if names:
            set_by_a_path |= set(lp.PATHS[path])
    assert set(lp.MATRIX) == set(lp.PATHS)
    assert not set_by_a_path & set(lp.COVERED_ELSEWHERE), "a switch a path sets needs no entry in COVERED_ELSEWHERE"
    read = _switches_read_by_the_library()
    untested = read - set_by_a_path - set(lp.COVERED_ELSEWHERE)
    assert not untested, f"no path of tests/launch_paths.py sets {sorted(untested)} and COVERED_ELSEWHERE does not name a test for them"
    stale = (set_by_a_path | set(lp.COVERED_ELSEWHERE)) - read
    assert not stale, f"the library no longer reads {sorted(stale)}"
    for name, test_file in lp.COVERED_ELSEWHERE.items():
        assert name in (ROOT / test_file).read_text(), f"{test_file} does not set {name}"


def test_every_problem_of_the_matrix_exists_and_mpc_paths_are_paths():
    for names in lp.MATRIX.values():
        assert set(names) <= set(lp._BUILDERS)
    assert set(lp.MPC_PATHS) <= set(lp.PATHS) and set(lp.BITWISE) <= set(lp.PATHS) and set(lp.MPC_CARRY_COUNT) <= set(lp.MPC_PATHS)
