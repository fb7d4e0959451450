"""The C++ client of plslam_lba_plan_optimize_dev: PLSLAM::LbaPlanSolver::optimizeOnDevice (plslam_amd/host/lba_rows.hpp) against
optimizeResident on the same plan, on committed cases of tests/golden/lba_lm_golden.npz -- compared inside
tests/cpp/test_lm_loop_ondev.cpp: the control flow exact, lambda to 1e-12, err to 1e-9 relative, the final state to 1e-9 of its scale
(the device's solve and SE(3) maps against the host's: rounding and libm).  Agreement with the reference's own text is
test_gpu_lba_optimize_dev.py's job."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from test_gpu_lba_lm import GOLD, ROOT, _write_problem


def _compile(tmp):
    exe = os.path.join(tmp, "test_lm_loop_ondev")
    cmd = [shutil.which("g++") or "g++", "-O2", "-std=c++17", "-pthread", "-Wall", "-Wextra", os.path.join(ROOT, "tests", "cpp", "test_lm_loop_ondev.cpp"),
           "-I" + os.path.join(ROOT, "include"), "-L" + os.path.join(ROOT, "plslam_amd", "lib"), "-lplslam_hip",
           "-L" + os.path.join(ROOT, "oracle"), "-lplslam_oracle",
           "-Wl,-rpath," + os.path.join(ROOT, "plslam_amd", "lib"), "-Wl,-rpath," + os.path.join(ROOT, "oracle"),
           "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib", "-lamdhip64", "-o", exe]
    subprocess.run(cmd, check=True)
    return exe


def test_the_on_device_loop_client_compiles_against_the_abi(tmp_path):
    """CPU: optimizeOnDevice and its test program compile and link against the C-ABI library."""
    _compile(str(tmp_path))


@pytest.mark.gpu
@pytest.mark.parametrize("name", ("main", "reject_later", "points_only"))
def test_optimize_on_device_agrees_with_optimize_resident(tmp_path, name):
    g = np.load(GOLD)
    exe = _compile(str(tmp_path))
    prob = str(tmp_path / "p.bin")
    _write_problem(prob, g, name)
    r = subprocess.run([exe, prob], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-1000:] + r.stderr[-2000:]
    assert ": agree" in r.stdout
