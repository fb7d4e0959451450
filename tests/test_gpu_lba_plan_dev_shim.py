"""The C++ client of the device-built LBA plan: PLSLAM::LbaPlanSolver's constructor from device columns and optimizeResident
(plslam_amd/host/lba_rows.hpp) against optimize() on the host-built plan, on the committed cases of tests/golden/lba_lm_golden.npz.
Trace (err, lambda, applied, iters, stop), x_kf and the final landmarks must be bitwise equal -- compared inside
tests/cpp/test_lm_loop_dev.cpp.  Agreement with the reference's own text is test_gpu_lba_lm.py's job."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from test_gpu_lba_lm import GOLD, ROOT, _write_problem


def _compile(tmp):
    exe = os.path.join(tmp, "test_lm_loop_dev")
    cmd = [shutil.which("g++") or "g++", "-O2", "-std=c++17", "-pthread", os.path.join(ROOT, "tests", "cpp", "test_lm_loop_dev.cpp"),
           "-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(ROOT, "include"), "-I/opt/rocm/include",
           "-L" + os.path.join(ROOT, "plslam_amd", "lib"), "-lplslam_hip", "-L" + os.path.join(ROOT, "oracle"), "-lplslam_oracle",
           "-Wl,-rpath," + os.path.join(ROOT, "plslam_amd", "lib"), "-Wl,-rpath," + os.path.join(ROOT, "oracle"),
           "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib", "-lamdhip64", "-o", exe]
    subprocess.run(cmd, check=True)
    return exe


def test_the_device_plan_client_compiles_against_the_abi(tmp_path):
    """CPU: the device-column constructor, optimizeResident and their test program compile and link against the C-ABI library."""
    _compile(str(tmp_path))


@pytest.mark.gpu
@pytest.mark.parametrize("name", ("main", "reject"))
def test_optimize_resident_equals_optimize_to_the_bit(tmp_path, name):
    g = np.load(GOLD)
    exe = _compile(str(tmp_path))
    prob = str(tmp_path / "p.bin")
    _write_problem(prob, g, name)
    r = subprocess.run([exe, prob], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-1000:] + r.stderr[-2000:]
    assert "equal to the bit" in r.stdout
