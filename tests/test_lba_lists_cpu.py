"""The host-built lists of the local BA (plslam_amd/csrc/lba_lists.hpp) without a GPU: tests/cpp/test_lba_lists.cpp is compiled with
g++ alone (no HIP header, no library) and run once; every case of it is one test here.  The same program built with the address and
undefined-behaviour sanitizers runs stand-alone and must come out clean."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = ["empty", "points_only", "lines_only", "both_kinds_null_padding", "exactly_one_chunk_of_points_no_padding",
         "more_than_one_chunk_of_a_kind", "fixed_keyframes"]


def _build_and_run(exe, extra):
    subprocess.run([shutil.which("g++") or "g++", "-O1", "-std=c++17", "-Wall", "-Wextra", "-Werror"] + extra +
                   [os.path.join(ROOT, "tests", "cpp", "test_lba_lists.cpp"), "-I" + os.path.join(ROOT, "plslam_amd", "csrc"), "-o", exe],
                   check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    res = dict(line.split(" ", 1)[::-1] for line in r.stdout.splitlines() if line.startswith(("PASS ", "FAIL ")))
    return {k.split(":")[0]: (v, k) for k, v in res.items()}, r.returncode, r.stderr


@pytest.fixture(scope="module")
def lists_results(tmp_path_factory):
    return _build_and_run(str(tmp_path_factory.mktemp("lba_lists") / "test_lba_lists"), [])


@pytest.mark.parametrize("case", CASES)
def test_lba_lists(lists_results, case):
    res = lists_results[0]
    assert case in res, f"{case}: the driver did not run it"
    assert res[case][0] == "PASS", res[case][1]


def test_lba_lists_driver_ran_every_case(lists_results):
    res, rc, _ = lists_results
    assert sorted(res) == sorted(CASES)
    assert rc == (0 if all(v[0] == "PASS" for v in res.values()) else 1)


def test_lba_lists_clean_under_sanitizers(tmp_path):
    res, rc, err = _build_and_run(str(tmp_path / "test_lba_lists_san"),
                                  ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"])
    assert rc == 0 and not err.strip(), err[-3000:]
    assert sorted(res) == sorted(CASES) and all(v[0] == "PASS" for v in res.values())
