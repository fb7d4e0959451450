"""Generates tests/golden/ref_calls_golden.npz.  Run from the repo root where oracle/_ref was built (needs the reference tree
at build time):
    python tests/golden/make_ref_calls_golden.py [--all]

Outputs of the REFERENCE ITSELF (its code compiled into oracle/_ref, see oracle/Makefile) for the cases of the pinning tests
in tests/test_oracle_pin.py that go through its helper _reference(): the popcount distances, the exact kNN search, computeLBD
with its tables and binaryConversion, updateAverageDescDir, the pose-only GN loops and the map<->KF visibility / gate loops
-- the latter also on the threshold cases of tests/map_gate_cases.py (tests/test_map_gate_cases_cpu.py), and the local-BA
observation loops on the row cases of tests/lba_row_cases.py (tests/test_lba_row_cases_cpu.py).
The tests are run with PLSLAM_RECORD_REF_CALLS set: each case writes the live output instead of comparing it, and this script
packs the records into one file.  Without oracle/_ref the same tests check the oracle against the recorded outputs.
"""
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "ref_calls_golden.npz")
TESTS = ["test_distance_pinned_to_reference_code", "test_knn2_distances_pinned_to_reference_mih_search",
         "test_lbd_compute_pinned_to_reference_code", "test_lbd_tables_and_binary_conversion_pinned_to_reference_code",
         "test_median_descriptor_pinned_to_reference_code", "test_pose_gn_loops_pinned_to_reference_source_text",
         "test_map2kf_visibility_and_gates_pinned_to_reference_source_text",
         # tests/test_map_gate_cases_cpu.py and tests/test_lba_row_cases_cpu.py
         "test_pinned_to_reference_source_text"]
FILES = ["test_oracle_pin.py", "test_map_gate_cases_cpu.py", "test_lba_row_cases_cpu.py"]


def main():
    sys.path.insert(0, ROOT)
    from oracle import oracle as O
    if O.ref_lib() is None:
        raise SystemExit("oracle/_ref is not built: nothing to record")
    with tempfile.TemporaryDirectory() as rec:
        cmd = [sys.executable, "-m", "pytest", "-q", "-p", "no:cacheprovider"] + \
            [f for f in (os.path.join(ROOT, "tests", x) for x in FILES) if os.path.exists(f)] + ["-k", " or ".join(TESTS)]
        subprocess.run(cmd, check=True, cwd=ROOT, env=dict(os.environ, PLSLAM_RECORD_REF_CALLS=rec))
        out = {}
        for f in sorted(os.listdir(rec)):
            with np.load(os.path.join(rec, f)) as z:
                out.update({k: z[k] for k in z.files})
    if "--all" not in sys.argv and os.path.exists(OUT):
        # keep every record the file already holds byte for byte (some hold bytes the reference never initialises: a fresh
        # recording would churn them) and add the new keys only; --all records everything afresh
        with np.load(OUT) as z:
            out.update({k: z[k] for k in z.files})
    np.savez_compressed(OUT, **out)
    print(f"{OUT}: {len(out)} arrays, {os.path.getsize(OUT)} bytes")
    # and the tests against the file just written
    subprocess.run(cmd, check=True, cwd=ROOT)


if __name__ == "__main__":
    main()
