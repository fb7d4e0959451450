"""A C++ client (tests/cpp/test_gba_dev_shim.cpp) runs one golden case (tests/gba_cases.py: ragged) through the resident route of
plslam_amd/host/gba.hpp -- the image packed by host/local_map.hpp, form_all + gather, the plan built on the device, the loop on
device state, the write-back into the image -- and through the existing host route gba::run in the same process: the poses, the
landmarks and the trace must be identical bit for bit."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import plslam_amd
from plslam_amd import synth

import gba_cases

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_cpp_resident_route_equals_the_host_route(tmp_path):
    lib = os.path.dirname(plslam_amd.LIB_PATH)
    exe = str(tmp_path / "test_gba_dev_shim")
    subprocess.run([shutil.which("g++") or "g++", "-O2", "-std=c++17", "-D__HIP_PLATFORM_AMD__",
                    os.path.join(ROOT, "tests", "cpp", "test_gba_dev_shim.cpp"), "-I" + os.path.join(ROOT, "include"), "-I/opt/rocm/include",
                    "-L" + lib, "-lplslam_hip", "-Wl,-rpath," + lib, "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib", "-lamdhip64", "-o", exe],
                   check=True)
    m = gba_cases.ragged()
    c = synth.EUROC
    (tmp_path / "meta.txt").write_text(f"{m['n_map_kf']} {m['npt']} {m['nls']} {c['fx']!r} {c['fy']!r} {c['cx']!r} {c['cy']!r}\n")
    for k, name, dt in (("T_kf_w", "T", np.float64), ("x_kf", "x", np.float64), ("Xw", "Xw", np.float64), ("Lw", "Lw", np.float64),
                        ("pt_obs", "pt_obs", np.int32), ("ls_obs", "ls_obs", np.int32), ("pt_uv", "pt_uv", np.float64),
                        ("ls_l", "ls_l", np.float64)):
        np.ascontiguousarray(m[k], dtype=dt).tofile(str(tmp_path / f"{name}.bin"))
    r = subprocess.run([exe, str(tmp_path)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip().startswith("solves") and "DIFFERENT" not in r.stdout
