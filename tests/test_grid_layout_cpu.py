"""The arithmetic of the windowed matcher (plslam_amd/csrc/match_grid_layout.hpp) without a GPU: tests/cpp/test_grid_layout.cpp is
compiled with g++ alone (no HIP header, no library) and run once; every case of it is one test here.  The same program built with
the address and undefined-behaviour sanitizers runs stand-alone and must come out clean."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = ["flat_bits", "scratch_layout", "lds_mode2", "modes_and_groups", "dense_layout", "store_capacity", "route"]


def _build_and_run(exe, extra):
    subprocess.run([shutil.which("g++") or "g++", "-O1", "-std=c++17", "-Wall", "-Wextra", "-Werror"] + extra +
                   [os.path.join(ROOT, "tests", "cpp", "test_grid_layout.cpp"), "-I" + os.path.join(ROOT, "plslam_amd", "csrc"), "-o", exe],
                   check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    res = dict(line.split(" ", 1)[::-1] for line in r.stdout.splitlines() if line.startswith(("PASS ", "FAIL ")))
    return {k.split(":")[0]: (v, k) for k, v in res.items()}, r.returncode, r.stderr


@pytest.fixture(scope="module")
def layout_results(tmp_path_factory):
    return _build_and_run(str(tmp_path_factory.mktemp("grid_layout") / "test_grid_layout"), [])


@pytest.mark.parametrize("case", CASES)
def test_grid_layout(layout_results, case):
    res = layout_results[0]
    assert case in res, f"{case}: the driver did not run it"
    assert res[case][0] == "PASS", res[case][1]


def test_grid_layout_driver_ran_every_case(layout_results):
    res, rc, _ = layout_results
    assert sorted(res) == sorted(CASES)
    assert rc == (0 if all(v[0] == "PASS" for v in res.values()) else 1)


def test_grid_layout_clean_under_sanitizers(tmp_path):
    res, rc, err = _build_and_run(str(tmp_path / "test_grid_layout_san"),
                                  ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"])
    assert rc == 0 and not err.strip(), err[-3000:]
    assert sorted(res) == sorted(CASES) and all(v[0] == "PASS" for v in res.values())
