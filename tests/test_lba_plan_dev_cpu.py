"""CPU tests of the device-built LBA plan's surface: the new entry points are exported and declared, the structs of the binding
have the header's layout, and the local map's C++ packer with applyLba compiles.  (The C++ client of the plan itself:
tests/test_gpu_lba_plan_dev_shim.py.)"""
import ctypes
import os
import re
import shutil
import subprocess

import plslam_amd
from plslam_amd import local_map as LM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("plslam_lba_plan_create_dev", "plslam_lba_plan_list_sizes", "plslam_lba_plan_lists", "plslam_local_map_apply_lba")


def test_the_new_symbols_are_exported_and_declared():
    lib = ctypes.CDLL(plslam_amd.LIB_PATH)
    L = plslam_amd.load()
    hdr = open(os.path.join(ROOT, "include", "plslam_hip.h")).read()
    for s in NEW:
        assert hasattr(lib, s), s
        assert s in plslam_amd.ABI_SYMBOLS and getattr(L, s).argtypes is not None, s
        assert re.search(r"\bint\s+" + s + r"\s*\(", hdr), s
    assert len(L.plslam_lba_plan_create_dev.argtypes) == 21


def test_the_grown_structs_keep_their_prefix(tmp_path):
    """plslam_local_map_buffers and plslam_local_map_counts grew at the END: the offsets a client compiled against the earlier
    header uses are unchanged, and the binding's structs have the header's sizes."""
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "plslam_hip.h"\nint main(void) {\n'
                   '  printf("%zu %zu %zu %zu %zu %zu %zu\\n", sizeof(plslam_local_map_buffers), offsetof(plslam_local_map_buffers, stream),\n'
                   '         offsetof(plslam_local_map_buffers, pt_moved), sizeof(plslam_local_map_counts),\n'
                   '         offsetof(plslam_local_map_counts, n_pt_moved), sizeof(plslam_local_map_lba_dst), sizeof(plslam_lba_list_sizes));\n'
                   '  return 0; }\n')
    exe = str(tmp_path / "layout")
    subprocess.run([shutil.which("gcc") or "gcc", "-std=c99", str(src), "-I" + os.path.join(ROOT, "include"), "-o", exe], check=True)
    got = [int(v) for v in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()]
    B, Cn = LM.LocalMapBuffers, LM.LocalMapCounts
    assert got == [ctypes.sizeof(B), B.stream.offset, B.pt_moved.offset, ctypes.sizeof(Cn), Cn.n_pt_moved.offset,
                   ctypes.sizeof(LM.LocalMapLbaDst), 11 * 4]
    assert B.stream.offset == 21 * 8 and B.pt_moved.offset == 22 * 8 and Cn.n_pt_moved.offset == 11 * 4      # the earlier structs' sizes


def test_the_local_map_packer_with_apply_lba_compiles(tmp_path):
    src = tmp_path / "use.cpp"
    src.write_text('#include "plslam_amd/host/local_map.hpp"\n#include "plslam_amd/host/lba_rows.hpp"\n'
                   'int use(PLSLAM::local_map::LocalMapIndex& ix, PLSLAM::LbaPlanSolver& s) { return ix.applyLba(s.handle(), 0.01); }\n')
    subprocess.run([shutil.which("g++") or "g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-c", str(src), "-D__HIP_PLATFORM_AMD__",
                    "-I" + ROOT, "-I" + os.path.join(ROOT, "include"), "-I/opt/rocm/include", "-o", str(tmp_path / "use.o")], check=True)
