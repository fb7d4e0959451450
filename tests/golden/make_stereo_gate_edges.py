#!/usr/bin/env python3
"""Writes tests/golden/stereo_gate_edges.npz: the threshold cases of tests/stereo_gate_cases.py at n_l = 65 and 257 -- inputs
and the outputs of the CPU restatement (oracle/plslam_oracle.c: plo_stereo_point_gate / plo_stereo_line_gate), disparities as
raw 64-bit words.  The device is checked against it with no oracle at run time (tests/test_gpu_stereo_gate_edges.py).
   python tests/golden/make_stereo_gate_edges.py"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from oracle import oracle as O  # noqa: E402
import stereo_gate_cases as C  # noqa: E402


def main():
    out, names, rows = {}, [], 0
    with np.errstate(all="ignore"):
        for c in C.all_cases():
            if c.n_l not in C.FIXTURE_SIZES:
                continue
            s12, disp, n = (O.stereo_point_gate if c.kind == "points" else O.stereo_line_gate)(*C.case_args(c))
            k = c.name
            names.append(k)
            rows += c.n_l
            out[k + ":m12"], out[k + ":f_l"], out[k + ":f_r"], out[k + ":th"] = c.m12, c.f_l, c.f_r, np.array(c.th, np.float64)
            out[k + ":stereo"], out[k + ":disp"], out[k + ":n"] = s12, disp, np.int32(n)
    out["names"] = np.array(names)
    path = os.path.join(ROOT, "tests", "golden", "stereo_gate_edges.npz")
    np.savez_compressed(path, **out)
    print("wrote", len(names), "cases,", rows, "rows,", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
