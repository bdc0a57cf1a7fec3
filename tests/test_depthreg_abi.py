"""No-GPU checks of include/vildepth.h (LiDAR depth association): libvilsolve.so exports every declared symbol, the ctypes mirror has the
C compiler's layout, vdepth_create refuses to run without a device, and none of the new kernels spills vector registers."""
import ctypes as C
import os
import re
import shutil
import subprocess
import tempfile

import numpy as np
import pytest

from mvil_fusion_amd import depthreg, lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LLVM = "/opt/rocm/lib/llvm/bin"


def test_library_exports_every_vdepth_symbol():
    so = lib.load_vilsolve()
    src = open(os.path.join(ROOT, "include", "vildepth.h")).read()
    syms = sorted(set(re.findall(r"\b(vdepth_[a-z_0-9]+)\s*\(", src)))
    assert syms == ["vdepth_create", "vdepth_debug_read", "vdepth_destroy", "vdepth_profile_enable", "vdepth_profile_read", "vdepth_register", "vdepth_set_cloud"], syms
    for s in syms:
        assert hasattr(so, s), "libvilsolve.so does not export %s" % s


def test_struct_layout_and_constants_match_header():
    prog = '#include <stdio.h>\n#include "vildepth.h"\nint main(void){printf("%zu %d %d %d\\n", sizeof(vdepth_summary), VDEPTH_BINS, VDEPTH_NUM_KERNELS, VDEPTH_MIN_SPHERE);return 0;}\n'
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "s.c"), "w").write(prog)
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), os.path.join(d, "s.c"), "-o", os.path.join(d, "s")])
        out = [int(v) for v in subprocess.check_output([os.path.join(d, "s")]).decode().split()]
    assert [C.sizeof(depthreg.VdepthSummary), depthreg.BINS, len(depthreg.KERNELS), depthreg.MIN_SPHERE] == out


def test_create_refuses_without_device():
    """No device (or, on a GPU machine, a device index that does not exist): VIL_ERR_DEVICE, there is no CPU fallback."""
    import torch
    with pytest.raises(depthreg.DepthRegError) as e:
        depthreg.DepthReg(lib.load_vilsolve(), device=1 << 20 if torch.cuda.is_available() else 0)
    assert e.value.status == -2


def test_view_matrices():
    """world_to_lidar inverts the pose; lidar_to_view ends in Tlc_: a point one metre in front of the camera comes out on the view
    frame's x axis."""
    c, s = np.cos(0.3), np.sin(0.3)
    R_wl, t_wl = np.array([[c, -s, 0], [s, c, 0], [0, 0, 1.0]]), np.array([1.0, -2.0, 0.5])
    R_lc, t_lc = depthreg.EXTRINSIC
    m1, m2 = depthreg.view_matrices(R_wl, t_wl, R_lc, t_lc)
    assert m1.dtype == np.float32 and m1.shape == (3, 4) and m2.dtype == np.float32 and m2.shape == (3, 4)
    p_l = np.array([3.0, 0.4, -0.2])
    assert np.allclose(m1[:, :3] @ (R_wl @ p_l + t_wl) + m1[:, 3], p_l, atol=1e-6)
    ahead = R_lc @ np.array([0.0, 0.0, 1.0]) + t_lc
    assert np.allclose(m2[:, :3] @ ahead + m2[:, 3], [1.0, 0.0, 0.0], atol=1e-6)
    right_down = R_lc @ np.array([0.2, 0.1, 1.0]) + t_lc
    assert np.allclose(m2[:, :3] @ right_down + m2[:, 3], [1.0, -0.2, -0.1], atol=1e-6)


@pytest.mark.skipif(not (os.path.exists(os.path.join(LLVM, "llvm-objdump")) and os.path.exists(os.path.join(LLVM, "llvm-readelf"))), reason="needs the ROCm LLVM tools")
def test_depth_kernels_do_not_spill_vector_registers():
    """Read from the code object's notes, as test_scanreg_abi.py does: no spill, no scratch, <= 128 vector registers, <= 160 kB of LDS."""
    with tempfile.TemporaryDirectory() as td:
        so = os.path.join(td, "lib.so"); shutil.copy(lib.LIB_PATH, so)
        subprocess.run([os.path.join(LLVM, "llvm-objdump"), "--offloading", so], cwd=td, check=True, capture_output=True)
        cos = [os.path.join(td, f) for f in os.listdir(td) if "gfx950" in f]
        assert cos, "no gfx950 code object in the library"
        seen = {}
        for co in cos:
            notes = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "--notes", co], check=True, capture_output=True, text=True).stdout
            chunks = notes.split(".name:")                  # a kernel's keys are sorted: .group_segment_fixed_size comes before its .name, the rest after
            for before, blk in zip(chunks[:-1], chunks[1:]):
                name = blk.split()[0]
                m = re.search(r"\.vgpr_spill_count:\s*(\d+)", blk); p = re.search(r"\.private_segment_fixed_size:\s*(\d+)", blk)
                v = re.search(r"\.vgpr_count:\s*(\d+)", blk); g = re.findall(r"\.group_segment_fixed_size:\s*(\d+)", before)
                if m and p and v and g: seen[name] = (int(m.group(1)), int(p.group(1)), int(v.group(1)), int(g[-1]))
    for k in depthreg.KERNELS:
        hit = [n for n in seen if k in n]
        assert len(hit) == 1, (k, sorted(seen))
        spill, scratch, vgprs, lds = seen[hit[0]]
        print(k, "vgprs", vgprs, "lds", lds)
        assert spill == 0 and scratch == 0, "%s spills %d vector registers (%d B of scratch per lane)" % (k, spill, scratch)
        assert vgprs <= 128 and lds <= 160 * 1024, (k, vgprs, lds)
