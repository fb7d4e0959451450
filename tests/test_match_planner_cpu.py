"""The match planner (plslam_amd/csrc/match_planner.hpp) without a GPU: tests/cpp/test_match_planner.cpp is compiled with g++ alone
(no HIP header, no library) and run once; every case of it is one test here."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = ["small_plan_wave_per_query", "mfma_forced_form_2", "mfma_forced_form_5", "auto_column_split_two_launches",
         "column_split_keep_prior_three_launches", "col_split_1_no_split", "throughput_plan_dealt_finalize", "directed_multi_window",
         "no_rows_no_columns_no_problems", "fuse_2_columns_fit", "fuse_2_columns_too_many", "post_fuse_2_16_row_blocks",
         "post_fuse_2_17_row_blocks", "device_row_count", "limits_and_arguments"]


@pytest.fixture(scope="module")
def planner_results(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("planner") / "test_match_planner")
    subprocess.run([shutil.which("g++") or "g++", "-O1", "-std=c++17", "-Wall", "-Wextra", "-Werror",
                    os.path.join(ROOT, "tests", "cpp", "test_match_planner.cpp"), "-I" + os.path.join(ROOT, "include"),
                    "-I" + os.path.join(ROOT, "plslam_amd", "csrc"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    res = dict(line.split(" ", 1)[::-1] for line in r.stdout.splitlines() if line.startswith(("PASS ", "FAIL ")))
    return {k.split(":")[0]: (v, k) for k, v in res.items()}, r.returncode


@pytest.mark.parametrize("case", CASES)
def test_match_planner(planner_results, case):
    res, _ = planner_results
    assert case in res, f"{case}: the driver did not run it"
    assert res[case][0] == "PASS", res[case][1]


def test_match_planner_driver_ran_every_case(planner_results):
    res, rc = planner_results
    assert sorted(res) == sorted(CASES)
    assert rc == (0 if all(v[0] == "PASS" for v in res.values()) else 1)
