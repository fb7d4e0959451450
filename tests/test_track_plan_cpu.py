"""The pure host planner of the tracker (plslam_amd/csrc/track_plan.hpp) without a GPU: tests/cpp/test_track_plan.cpp is compiled
with g++ alone (no HIP header, no library) against plslam_amd/csrc and include only.  Its hand cases run once, every case one
test here; the same program built with the address and undefined-behaviour sanitizers runs stand-alone and must come out
clean."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HAND = ["capacities_are_the_sums_of_the_prev_counts", "b_zero_is_ok_and_plans_nothing", "null_arguments_and_negative_sizes_are_einval",
        "a_null_array_is_refused_only_where_rows_exist", "counts_and_batch_over_the_limits_are_erange",
        "the_largest_batch_of_the_largest_pairs_stays_under_2_31_rows", "layout_every_array_on_256_bytes_in_order_without_overlap",
        "layout_a_kind_without_rows_keeps_distinct_addresses", "launches_one_workgroup_per_pair_and_kind_one_for_the_scan",
        "scan_chunks_cover_every_pair_once"]
SANITIZE = ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]


def _build(exe, extra):
    subprocess.run([shutil.which("g++") or "g++", "-O1", "-std=c++17", "-Wall", "-Wextra", "-Werror"] + extra +
                   [os.path.join(ROOT, "tests", "cpp", "test_track_plan.cpp"), "-I" + os.path.join(ROOT, "plslam_amd", "csrc"),
                    "-I" + os.path.join(ROOT, "include"), "-o", exe], check=True)
    return exe


def _hand(exe):
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    res = dict(line.split(" ", 1)[::-1] for line in r.stdout.splitlines() if line.startswith(("PASS ", "FAIL ")))
    return {k.split(":")[0]: (v, k) for k, v in res.items()}, r.returncode, r.stderr


@pytest.fixture(scope="module")
def hand_results(tmp_path_factory):
    return _hand(_build(str(tmp_path_factory.mktemp("track_plan") / "test_track_plan"), []))


@pytest.mark.parametrize("case", HAND)
def test_track_plan_hand_case(hand_results, case):
    res = hand_results[0]
    assert case in res, f"{case}: the driver did not run it"
    assert res[case][0] == "PASS", res[case][1]


def test_track_plan_driver_ran_exactly_the_listed_cases(hand_results):
    res, rc, _ = hand_results
    assert sorted(res) == sorted(HAND)
    assert rc == (0 if all(v[0] == "PASS" for v in res.values()) else 1)


def test_track_plan_clean_under_sanitizers(tmp_path):
    """The hand cases in a build of the program with the sanitizers: run as a program, nothing is loaded into Python"""
    res, rc, err = _hand(_build(str(tmp_path / "test_track_plan_san"), SANITIZE))
    assert rc == 0 and not err.strip(), err[-3000:]
    assert sorted(res) == sorted(HAND) and all(v[0] == "PASS" for v in res.values())


def test_planner_header_needs_no_hip():
    """track_plan.hpp and what it includes name no HIP header and not the library's internal one"""
    csrc = os.path.join(ROOT, "plslam_amd", "csrc")
    for path in (os.path.join(csrc, "track_plan.hpp"), os.path.join(csrc, "match_tables.hpp"), os.path.join(ROOT, "include", "plslam_track.h")):
        with open(path) as f:
            inc = [l.split()[1].strip('<>"') for l in f if l.startswith("#include")]
        assert not [i for i in inc if i.startswith("hip/") or i == "common.hpp"], (path, inc)
