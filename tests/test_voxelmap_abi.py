"""No-GPU checks of include/vilvgicp_voxel.h (the device builder of the target voxel map, reached through include/vilvgicp.h):
libvilsolve.so exports every declared symbol, the ctypes mirror of vgicp_voxels has the C compiler's layout, the constants agree, and
none of the builder's kernels spills vector registers."""
import ctypes as C
import os
import re
import shutil
import subprocess
import tempfile

import pytest

from mvil_fusion_amd import lib, vgicp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LLVM = "/opt/rocm/lib/llvm/bin"


def test_library_exports_every_declared_symbol():
    so = lib.load_vilsolve()
    src = open(os.path.join(ROOT, "include", "vilvgicp_voxel.h")).read()
    syms = sorted(set(re.findall(r"\b(vgicp_[a-z_0-9]+)\s*\(", src)))
    assert syms == ["vgicp_build_profile_enable", "vgicp_build_profile_read", "vgicp_promote_source", "vgicp_read_voxels", "vgicp_set_voxel_builder"], syms
    for s in syms:
        assert hasattr(so, s), "libvilsolve.so does not export %s" % s
    assert '#include "vilvgicp_voxel.h"' in open(os.path.join(ROOT, "include", "vilvgicp.h")).read()      # a caller includes vilvgicp.h alone


def test_struct_layout_and_constants_match_header():
    """Compiled against vilvgicp.h only: the additions arrive through it."""
    fields = [f for f, _ in vgicp.VgicpVoxels._fields_]
    consts = ["VGICP_BUILD_HOST", "VGICP_BUILD_DEVICE", "VGICP_BUILD_KERNELS", "VIL_ERR_INVALID_ARGUMENT", "VIL_ERR_NON_FINITE"]
    prog = ('#include <stdio.h>\n#include <stddef.h>\n#include "vilsolve.h"\n#include "vilvgicp.h"\nint main(void){printf("%zu ", sizeof(vgicp_voxels));' +
            "".join('printf("%%zu ", offsetof(vgicp_voxels, %s));' % f for f in fields) + "".join('printf("%%d ", (int)%s);' % c for c in consts) + 'printf("\\n");return 0;}\n')
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "s.c"), "w").write(prog)
        subprocess.check_call(["gcc", "-std=c99", "-pedantic-errors", "-I", os.path.join(ROOT, "include"), os.path.join(d, "s.c"), "-o", os.path.join(d, "s")])
        out = [int(v) for v in subprocess.check_output([os.path.join(d, "s")]).decode().split()]
    mine = [C.sizeof(vgicp.VgicpVoxels)] + [getattr(vgicp.VgicpVoxels, f).offset for f in fields]
    mine += [vgicp.BUILD_HOST, vgicp.BUILD_DEVICE, len(vgicp.BUILD_KERNELS), vgicp.ERR_INVALID_ARGUMENT, vgicp.ERR_NON_FINITE]
    assert mine == out
    assert C.sizeof(vgicp.VgicpVoxels) == 48


def test_the_wrapper_has_the_new_calls():
    for name in ("set_voxel_builder", "promote_source", "read_voxels", "build_profile_enable", "build_profile_read"):
        assert callable(getattr(vgicp.Vgicp, name))


@pytest.mark.skipif(not (os.path.exists(os.path.join(LLVM, "llvm-objdump")) and os.path.exists(os.path.join(LLVM, "llvm-readelf"))), reason="needs the ROCm LLVM tools")
def test_builder_kernels_do_not_spill_vector_registers():
    """From the code object's notes, as tests/test_cloud_abi.py reads them: no spill, no scratch, at most 64 vector registers."""
    with tempfile.TemporaryDirectory() as td:
        so = os.path.join(td, "lib.so"); shutil.copy(lib.LIB_PATH, so)
        subprocess.run([os.path.join(LLVM, "llvm-objdump"), "--offloading", so], cwd=td, check=True, capture_output=True)
        cos = [os.path.join(td, f) for f in os.listdir(td) if "gfx950" in f]
        assert cos, "no gfx950 code object in the library"
        seen = {}
        for co in cos:
            notes = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "--notes", co], check=True, capture_output=True, text=True).stdout
            for blk in notes.split(".name:")[1:]:
                name = blk.split()[0]
                m = re.search(r"\.vgpr_spill_count:\s*(\d+)", blk); p = re.search(r"\.private_segment_fixed_size:\s*(\d+)", blk); v = re.search(r"\.vgpr_count:\s*(\d+)", blk)
                if m and p and v: seen[name] = (int(m.group(1)), int(p.group(1)), int(v.group(1)))
    for k in vgicp.BUILD_KERNELS:
        hit = [n for n in seen if re.search(r"\d%s[A-Z]" % k, n)]
        assert len(hit) == 1, (k, hit)
        spill, scratch, vgprs = seen[hit[0]]
        assert spill == 0 and scratch == 0, "%s spills %d vector registers (%d B of scratch per lane)" % (k, spill, scratch)
        assert vgprs <= 64, (k, vgprs)
