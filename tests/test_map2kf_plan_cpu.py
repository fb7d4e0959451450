"""The pure host planner of the map<->keyframe and keyframe<->keyframe drivers (plslam_amd/csrc/map2kf_plan.hpp) without a GPU:
tests/cpp/test_map2kf_plan.cpp is compiled with g++ alone (no HIP header, no library) against plslam_amd/csrc and include, and
linked with the project's restatement of the reference (oracle/plslam_oracle.c) for the grid fill.  Its hand cases run once,
every case one test here; the same program built with the address and undefined-behaviour sanitizers runs stand-alone and must
come out clean."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HAND = ["line_cells_steep", "line_cells_right_to_left", "line_cells_horizontal_last_x_excluded", "line_cells_zero_length",
        "line_cells_negative_coordinates", "line_cells_diagonal_against_oracle",
        "point_cells_nan_and_huge_are_dropped", "point_cells_border_column_and_row_dropped", "point_cells_corner_cells_kept",
        "csr_fill_push_order_and_sizes",
        "grid_tables_points_with_and_without_sel", "grid_tables_lines_dir2_and_three_cells", "grid_tables_points_against_oracle",
        "line_grid_bound_cases",
        "once_layout_sweep", "once_layout_is_the_carving_it_replaces", "once_layout_written_down", "step_layout", "grid_path_layout",
        "kf2kf_layout", "stage_once_image_contents", "fill_grid_problem_fields",
        "map2kf_entry_table", "kf2kf_entry_table", "entry_apply_writes_what_the_entry_says",
        "kf2kf_table_all_combinations", "decisions_thresholds", "both_known_needs_every_condition"]
SANITIZE = ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]


def _build(exe, extra):
    inc = ["-I" + os.path.join(ROOT, d) for d in (os.path.join("plslam_amd", "csrc"), "include", "oracle")]
    obj = exe + "_oracle.o"
    subprocess.run([shutil.which("gcc") or "gcc", "-O1", "-std=c11", "-ffp-contract=off", "-mpopcnt", "-msse4.2"] + extra +
                   ["-c", os.path.join(ROOT, "oracle", "plslam_oracle.c"), "-o", obj], check=True)
    subprocess.run([shutil.which("g++") or "g++", "-O1", "-std=c++17", "-Wall", "-Wextra", "-Werror"] + extra +
                   [os.path.join(ROOT, "tests", "cpp", "test_map2kf_plan.cpp"), obj] + inc + ["-o", exe, "-lm", "-lpthread"], check=True)
    return exe


def _hand(exe):
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    res = dict(line.split(" ", 1)[::-1] for line in r.stdout.splitlines() if line.startswith(("PASS ", "FAIL ")))
    return {k.split(":")[0]: (v, k) for k, v in res.items()}, r.returncode, r.stderr


@pytest.fixture(scope="module")
def hand_results(tmp_path_factory):
    return _hand(_build(str(tmp_path_factory.mktemp("map2kf_plan") / "test_map2kf_plan"), []))


@pytest.mark.parametrize("case", HAND)
def test_map2kf_plan_hand_case(hand_results, case):
    res = hand_results[0]
    assert case in res, f"{case}: the driver did not run it"
    assert res[case][0] == "PASS", res[case][1]


def test_map2kf_plan_driver_ran_exactly_the_listed_cases(hand_results):
    res, rc, _ = hand_results
    assert sorted(res) == sorted(HAND)
    assert rc == (0 if all(v[0] == "PASS" for v in res.values()) else 1)


def test_map2kf_plan_clean_under_sanitizers(tmp_path):
    """The hand cases in a build of the program with the sanitizers: run as a program, nothing is loaded into Python"""
    res, rc, err = _hand(_build(str(tmp_path / "test_map2kf_plan_san"), SANITIZE))
    assert rc == 0 and not err.strip(), err[-3000:]
    assert sorted(res) == sorted(HAND) and all(v[0] == "PASS" for v in res.values())


def test_planner_header_needs_no_hip():
    """map2kf_plan.hpp and what it includes name no HIP header and not the library's internal one"""
    csrc = os.path.join(ROOT, "plslam_amd", "csrc")
    for name in ("map2kf_plan.hpp", "match_grid_layout.hpp", "match_tables.hpp"):
        with open(os.path.join(csrc, name)) as f:
            inc = [l.split()[1].strip('<>"') for l in f if l.startswith("#include")]
        assert not [i for i in inc if i.startswith("hip/") or i == "common.hpp"], (name, inc)
