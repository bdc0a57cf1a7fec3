"""No-GPU checks of include/vilfront.h (processLidar as one resident call): libvilsolve.so exports every declared symbol and nothing of the
three hand-over stages, the ctypes mirrors have the C compiler's layout, vfront_create refuses to run without a device, and none of the
new kernels spills vector registers."""
import ctypes as C
import os
import re
import shutil
import subprocess
import tempfile

import pytest

from mvil_fusion_amd import lib, lidarfront

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LLVM = "/opt/rocm/lib/llvm/bin"
PUBLIC = ["vfront_create", "vfront_debug_read", "vfront_default_options", "vfront_destroy", "vfront_profile_enable", "vfront_profile_read", "vfront_push_scan",
          "vfront_read_deskewed", "vfront_reset", "vfront_set_grid"]


def test_library_exports_every_vfront_symbol():
    so = lib.load_vilsolve()
    src = open(os.path.join(ROOT, "include", "vilfront.h")).read()
    syms = sorted(set(re.findall(r"\b(vfront_[a-z_0-9]+)\s*\(", src)))
    assert syms == PUBLIC, syms
    for s in syms:
        assert hasattr(so, s), "libvilsolve.so does not export %s" % s


def test_the_stages_are_not_exported():
    """vfront_push_scan reaches the filter, the registration and the fitness contexts through csrc/vilcloud_stage.hpp, vilvgicp_stage.hpp
    and villoop_stage.hpp: hidden C++ symbols, no new entry point of those rows."""
    out = subprocess.run(["nm", "-D", "--defined-only", lib.LIB_PATH], check=True, capture_output=True, text=True).stdout
    names = [l.split()[-1] for l in out.splitlines() if l.strip()]
    assert sorted(n for n in names if "vfront" in n) == PUBLIC
    for ns in ("vilcloud_stage", "vilvgicp_stage", "villoop_stage"):
        assert not [n for n in names if ns in n], "the functions of %s are exported" % ns
    for h in ("vilcloud_stage.hpp", "vilvgicp_stage.hpp", "villoop_stage.hpp"):
        text = open(os.path.join(ROOT, "mvil-fusion_amd", "csrc", h)).read()
        decl = [l for l in text.splitlines() if re.match(r"^(__attribute__|int |bool )", l)]
        assert decl and all('visibility("hidden")' in l for l in decl), (h, decl)


def _offsets(struct, prefix=""):
    return [(prefix + f, getattr(struct, f).offset) for f, _ in struct._fields_]


def test_struct_layout_constants_and_defaults_match_header():
    structs = [("vfront_motion", lidarfront.VfrontMotion), ("vfront_options", lidarfront.VfrontOptions), ("vfront_summary", lidarfront.VfrontSummary)]
    fields = [(n, f) for n, s in structs for f, _ in s._fields_]
    consts = ["VFRONT_NUM_KERNELS", "VFRONT_KNN", "VFRONT_DBG_DESKEWED", "VFRONT_DBG_FILTERED", "VIL_ERR_INVALID_ARGUMENT", "VIL_ERR_DEVICE", "VIL_ERR_NON_FINITE"]
    prog = ('#include <stdio.h>\n#include <stddef.h>\n#include "vilfront.h"\nint main(void){' + "".join('printf("%%zu ", sizeof(%s));' % n for n, _ in structs) +
            "".join('printf("%%zu ", offsetof(%s, %s));' % sf for sf in fields) + "".join('printf("%%d ", (int)%s);' % c for c in consts) + 'printf("\\n");return 0;}\n')
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "s.c"), "w").write(prog)
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), os.path.join(d, "s.c"), "-o", os.path.join(d, "s")])
        out = [int(v) for v in subprocess.check_output([os.path.join(d, "s")]).decode().split()]
    mine = [C.sizeof(s) for _, s in structs] + [getattr(s, f).offset for _, s in structs for f, _ in s._fields_]
    mine += [len(lidarfront.KERNELS), lidarfront.KNN, lidarfront.DBG_DESKEWED, lidarfront.DBG_FILTERED, lidarfront.ERR_INVALID_ARGUMENT, lidarfront.ERR_DEVICE,
             lidarfront.ERR_NON_FINITE]
    assert mine == out
    so = lib.load_vilsolve()
    o = lidarfront.default_options(so)                       # runs without a device
    assert (o.deskew, o.hist_size, o.lidar_time_step, o.min_distance, o.max_distance, o.resolution, o.leaf) == (1, 512, 0.1, 0.5, 70.0, 0.5, C.c_float(0.3).value)
    from mvil_fusion_amd import vgicp
    r = vgicp.VgicpOptions()
    f = so.vgicp_default_options; f.restype = None
    f(C.byref(r))
    assert lidarfront.summary_bytes(o.reg) == lidarfront.summary_bytes(r)
    assert lidarfront.default_options(so, hist_size=64, max_iterations=7).reg.max_iterations == 7


def test_create_refuses_without_device():
    """No device (or, on a GPU machine, a device index that does not exist): VIL_ERR_DEVICE, there is no CPU fallback."""
    import torch
    with pytest.raises(lidarfront.LidarFrontError) as e:
        lidarfront.LidarFront(lib.load_vilsolve(), max_scan_points=64, device=1 << 20 if torch.cuda.is_available() else 0)
    assert e.value.status == lidarfront.ERR_DEVICE
    for bad in (0, -1, (1 << 27) + 1):
        with pytest.raises(lidarfront.LidarFrontError) as e:
            lidarfront.LidarFront(lib.load_vilsolve(), max_scan_points=bad)
        assert e.value.status == lidarfront.ERR_INVALID_ARGUMENT, bad


@pytest.mark.skipif(not (os.path.exists(os.path.join(LLVM, "llvm-objdump")) and os.path.exists(os.path.join(LLVM, "llvm-readelf"))), reason="needs the ROCm LLVM tools")
def test_front_kernels_do_not_spill_vector_registers():
    """Read from the code object's notes, as test_cloud_abi.py does: no spill, no scratch, <= 128 vector registers."""
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
    for k in lidarfront.KERNELS:
        hit = [n for n in seen if k in n]
        assert len(hit) == 1, (k, sorted(seen))
        spill, scratch, vgprs, lds = seen[hit[0]]
        print(k, "vgprs", vgprs, "lds", lds)
        assert spill == 0 and scratch == 0, "%s spills %d vector registers (%d B of scratch per lane)" % (k, spill, scratch)
        assert vgprs <= 128 and lds <= 160 * 1024, (k, vgprs, lds)
