"""No-GPU checks of include/vilcloud.h (the device-resident depth cloud and filter A): libvilsolve.so exports every declared symbol and
nothing of the hand-over stage, the ctypes mirrors have the C compiler's layout, vcloud_create refuses to run without a device, and none of
the new kernels spills vector registers."""
import ctypes as C
import os
import re
import shutil
import subprocess
import tempfile

import pytest

from mvil_fusion_amd import cloud, lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LLVM = "/opt/rocm/lib/llvm/bin"


def test_library_exports_every_vcloud_symbol():
    so = lib.load_vilsolve()
    src = open(os.path.join(ROOT, "include", "vilcloud.h")).read()
    syms = sorted(set(re.findall(r"\b(vcloud_[a-z_0-9]+)\s*\(", src)))
    assert syms == ["vcloud_create", "vcloud_debug_read", "vcloud_default_options", "vcloud_destroy", "vcloud_filter", "vcloud_profile_enable", "vcloud_profile_read",
                    "vcloud_publish", "vcloud_push_scan", "vcloud_read_cloud", "vcloud_reset"], syms
    for s in syms:
        assert hasattr(so, s), "libvilsolve.so does not export %s" % s


def test_the_hand_over_stage_is_not_exported():
    """vcloud_publish reaches the depth context through csrc/vildepth_stage.hpp: hidden C++ symbols, no new vdepth_* entry point."""
    out = subprocess.run(["nm", "-D", "--defined-only", lib.LIB_PATH], check=True, capture_output=True, text=True).stdout
    names = [l.split()[-1] for l in out.splitlines() if l.strip()]
    assert sorted(n for n in names if n.startswith("vdepth_")) == ["vdepth_create", "vdepth_debug_read", "vdepth_destroy", "vdepth_profile_enable", "vdepth_profile_read",
                                                                  "vdepth_register", "vdepth_set_cloud"]
    assert not [n for n in names if "vildepth_stage" in n], "the stage functions are exported"
    assert sorted(n for n in names if "vcloud" in n) == sorted("vcloud_" + s for s in ("create", "debug_read", "default_options", "destroy", "filter", "profile_enable",
                                                                                       "profile_read", "publish", "push_scan", "read_cloud", "reset"))


def test_struct_layout_constants_and_defaults_match_header():
    fields = [("vcloud_options", f) for f, _ in cloud.VcloudOptions._fields_] + [("vcloud_summary", f) for f, _ in cloud.VcloudSummary._fields_]
    consts = ["VCLOUD_NUM_KERNELS", "VCLOUD_MAX_HIST", "VCLOUD_MAX_SCANS", "VCLOUD_DBG_SCAN_DS", "VCLOUD_DBG_SCAN_WORLD", "VCLOUD_DBG_FUSED", "VIL_ERR_INVALID_ARGUMENT",
              "VIL_ERR_DEVICE", "VIL_ERR_CAPACITY"]
    prog = ('#include <stdio.h>\n#include <stddef.h>\n#include "vilcloud.h"\nint main(void){printf("%zu %zu ", sizeof(vcloud_options), sizeof(vcloud_summary));' +
            "".join('printf("%%zu ", offsetof(%s, %s));' % sf for sf in fields) + "".join('printf("%%d ", (int)%s);' % c for c in consts) + 'printf("\\n");return 0;}\n')
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "s.c"), "w").write(prog)
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), os.path.join(d, "s.c"), "-o", os.path.join(d, "s")])
        out = [int(v) for v in subprocess.check_output([os.path.join(d, "s")]).decode().split()]
    mine = [C.sizeof(cloud.VcloudOptions), C.sizeof(cloud.VcloudSummary)]
    mine += [getattr(cloud.VcloudOptions, f).offset for f, _ in cloud.VcloudOptions._fields_] + [getattr(cloud.VcloudSummary, f).offset for f, _ in cloud.VcloudSummary._fields_]
    mine += [len(cloud.KERNELS), cloud.MAX_HIST, cloud.MAX_SCANS, cloud.DBG_SCAN_DS, cloud.DBG_SCAN_WORLD, cloud.DBG_FUSED, cloud.ERR_INVALID_ARGUMENT, cloud.ERR_DEVICE,
             cloud.ERR_CAPACITY]
    assert mine == out
    o = cloud.default_options(lib.load_vilsolve())          # runs without a device
    assert (o.leaf_scan, o.leaf_cloud, o.hist_size, o.max_coord, o.max_ratio, o.window_s) == (C.c_float(0.2).value, C.c_float(0.1).value, 512, 25.0, 10.0, 5.0)
    assert cloud.default_options(lib.load_vilsolve(), hist_size=64).hist_size == 64


def test_create_refuses_without_device():
    """No device (or, on a GPU machine, a device index that does not exist): VIL_ERR_DEVICE, there is no CPU fallback."""
    import torch
    with pytest.raises(cloud.CloudError) as e:
        cloud.DepthCloud(lib.load_vilsolve(), max_scan_points=64, max_scans=2, device=1 << 20 if torch.cuda.is_available() else 0)
    assert e.value.status == cloud.ERR_DEVICE
    for bad in (dict(max_scan_points=0), dict(max_scans=0), dict(max_scans=cloud.MAX_SCANS + 1), dict(max_scan_points=1 << 24, max_scans=16)):
        with pytest.raises(cloud.CloudError) as e:
            cloud.DepthCloud(lib.load_vilsolve(), **{**dict(max_scan_points=64, max_scans=2), **bad})
        assert e.value.status == cloud.ERR_INVALID_ARGUMENT, bad


@pytest.mark.skipif(not (os.path.exists(os.path.join(LLVM, "llvm-objdump")) and os.path.exists(os.path.join(LLVM, "llvm-readelf"))), reason="needs the ROCm LLVM tools")
def test_cloud_kernels_do_not_spill_vector_registers():
    """Read from the code object's notes, as test_depthreg_abi.py does: no spill, no scratch, <= 128 vector registers, <= 160 kB of LDS."""
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
    for k in cloud.KERNELS:
        hit = [n for n in seen if k in n]
        assert len(hit) == 1, (k, sorted(seen))
        spill, scratch, vgprs, lds = seen[hit[0]]
        print(k, "vgprs", vgprs, "lds", lds)
        assert spill == 0 and scratch == 0, "%s spills %d vector registers (%d B of scratch per lane)" % (k, spill, scratch)
        assert vgprs <= 128 and lds <= 160 * 1024, (k, vgprs, lds)
