"""The pure host half of the map insert (plslam_amd/csrc/map_insert_plan.hpp) without a GPU: tests/cpp/test_map_insert_plan.cpp
is compiled with g++ alone (no HIP header, no library) against plslam_amd/csrc and include.  Its hand cases run once, every case
one test here; the same program built with the address and undefined-behaviour sanitizers runs stand-alone and must come out
clean."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HAND = ["accepts_both_modes", "null_arguments", "slots_out_of_range", "destination_is_a_source", "kind_arguments", "table_length",
        "capacities", "precedence", "events_and_bounds", "layout_at_the_tile_edges", "pack_into_an_exact_buffer"]
SANITIZE = ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]


def _build(exe, extra):
    inc = ["-I" + os.path.join(ROOT, d) for d in (os.path.join("plslam_amd", "csrc"), "include")]
    subprocess.run([shutil.which("g++") or "g++", "-O1", "-std=c++17", "-Wall", "-Wextra", "-Werror"] + extra +
                   [os.path.join(ROOT, "tests", "cpp", "test_map_insert_plan.cpp")] + inc + ["-o", exe], check=True)
    return exe


def _hand(exe):
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    res = dict(line.split(" ", 1)[::-1] for line in r.stdout.splitlines() if line.startswith(("PASS ", "FAIL ")))
    return {k.split(":")[0]: (v, k) for k, v in res.items()}, r.returncode, r.stderr


@pytest.fixture(scope="module")
def hand_results(tmp_path_factory):
    return _hand(_build(str(tmp_path_factory.mktemp("map_insert_plan") / "test_map_insert_plan"), []))


@pytest.mark.parametrize("case", HAND)
def test_map_insert_plan_hand_case(hand_results, case):
    res = hand_results[0]
    assert case in res, f"{case}: the driver did not run it"
    assert res[case][0] == "PASS", res[case][1]


def test_map_insert_plan_driver_ran_exactly_the_listed_cases(hand_results):
    res, rc, _ = hand_results
    assert sorted(res) == sorted(HAND)
    assert rc == (0 if all(v[0] == "PASS" for v in res.values()) else 1)


def test_map_insert_plan_clean_under_sanitizers(tmp_path):
    """The hand cases in a build of the program with the sanitizers: run as a program, nothing is loaded into Python"""
    res, rc, err = _hand(_build(str(tmp_path / "test_map_insert_plan_san"), SANITIZE))
    assert rc == 0 and not err.strip(), err[-3000:]
    assert sorted(res) == sorted(HAND) and all(v[0] == "PASS" for v in res.values())


def test_planner_header_needs_no_hip():
    """map_insert_plan.hpp and what it includes name no HIP header and not the library's internal one"""
    csrc = os.path.join(ROOT, "plslam_amd", "csrc")
    for name in ("map_insert_plan.hpp", "map_image.hpp", "match_tables.hpp"):
        with open(os.path.join(csrc, name)) as f:
            inc = [l.split()[1].strip('<>"') for l in f if l.startswith("#include")]
        assert not [i for i in inc if i.startswith("hip/") or i == "common.hpp"], (name, inc)
