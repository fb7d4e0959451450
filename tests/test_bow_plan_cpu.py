"""The pure host planner of the bag of words (plslam_amd/csrc/bow_plan.hpp) without a GPU: tests/cpp/test_bow_plan.cpp is compiled
with g++ alone (no HIP header, no library) against plslam_amd/csrc and include only.  Its hand cases run once, every case one
test here; the same program built with the address and undefined-behaviour sanitizers runs stand-alone and must come out
clean."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HAND = ["flatten_the_three_node_tree_written_out_by_hand", "flatten_refuses_what_the_gpu_validation_test_refuses",
        "flatten_refusals_no_gpu_test_reaches", "flatten_shuffled_records_keep_children_in_record_order_not_id_order",
        "flatten_records_in_reverse_order", "flatten_complete_trees_of_1227_1228_1229_nodes_stage_min_of_n_and_1228",
        "flatten_a_parents_children_straddle_position_1228", "flatten_a_two_node_cycle_off_the_root_is_refused_by_the_count",
        "transform_offsets_first_nonzero_decreasing_and_the_largest_set", "transform_nsets_zero_is_ok_and_reads_nothing",
        "transform_layout_slices_on_256_bytes_in_order_and_disjoint", "transform_dev_argument_and_alignment_rules",
        "geometry_lds_bytes_grids_and_their_limits", "db_initial_capacities_for_hints_0_4_16_17", "db_an_insert_that_grows_nothing",
        "db_the_table_grows_at_kf_idx_equal_to_cap_kf", "db_a_pool_is_full_at_used_plus_n_equal_cap_and_grows_one_beyond",
        "db_kf_idx_jumps_from_3_to_1000", "db_a_mode_without_points_zeroes_n_p_and_never_plans_a_point_pool",
        "db_a_plan_leaves_the_state_untouched_until_commit", "db_the_2_31_refusal_plans_no_growth",
        "db_keep_is_what_is_in_use_not_the_capacity", "db_inserting_an_index_again_overwrites_its_reservation_and_advances_used",
        "db_score_plan_capacities_are_the_maximum_over_the_queries",
        "db_host_insert_layout_alive_bytes_upload_before_the_words_row_of_doubles", "db_insert_argument_rules"]
SANITIZE = ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]


def _build(exe, extra):
    subprocess.run([shutil.which("g++") or "g++", "-O1", "-std=c++17", "-Wall", "-Wextra", "-Werror"] + extra +
                   [os.path.join(ROOT, "tests", "cpp", "test_bow_plan.cpp"), "-I" + os.path.join(ROOT, "plslam_amd", "csrc"),
                    "-I" + os.path.join(ROOT, "include"), "-o", exe], check=True)
    return exe


def _hand(exe):
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    res = dict(line.split(" ", 1)[::-1] for line in r.stdout.splitlines() if line.startswith(("PASS ", "FAIL ")))
    return {k.split(":")[0]: (v, k) for k, v in res.items()}, r.returncode, r.stderr


@pytest.fixture(scope="module")
def hand_results(tmp_path_factory):
    return _hand(_build(str(tmp_path_factory.mktemp("bow_plan") / "test_bow_plan"), []))


@pytest.mark.parametrize("case", HAND)
def test_bow_plan_hand_case(hand_results, case):
    res = hand_results[0]
    assert case in res, f"{case}: the driver did not run it"
    assert res[case][0] == "PASS", res[case][1]


def test_bow_plan_driver_ran_exactly_the_listed_cases(hand_results):
    res, rc, _ = hand_results
    assert sorted(res) == sorted(HAND)
    assert rc == (0 if all(v[0] == "PASS" for v in res.values()) else 1)


def test_bow_plan_clean_under_sanitizers(tmp_path):
    """The hand cases in a build of the program with the sanitizers: run as a program, nothing is loaded into Python"""
    res, rc, err = _hand(_build(str(tmp_path / "test_bow_plan_san"), SANITIZE))
    assert rc == 0 and not err.strip(), err[-3000:]
    assert sorted(res) == sorted(HAND) and all(v[0] == "PASS" for v in res.values())


def test_planner_header_needs_no_hip():
    """bow_plan.hpp and what it includes name no HIP header and not the library's internal one"""
    csrc = os.path.join(ROOT, "plslam_amd", "csrc")
    for path in (os.path.join(csrc, "bow_plan.hpp"), os.path.join(csrc, "match_tables.hpp"), os.path.join(ROOT, "include", "plslam_hip.h")):
        with open(path) as f:
            inc = [l.split()[1].strip('<>"') for l in f if l.startswith("#include")]
        assert not [i for i in inc if i.startswith("hip/") or i == "common.hpp"], (path, inc)
