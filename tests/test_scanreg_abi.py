"""No-GPU checks of include/vilscan.h (LOAM feature extraction): libvilsolve.so exports every declared symbol, the ctypes mirrors have the
C compiler's layout, vscan_create refuses to run without a device, and none of the new kernels spills vector registers."""
import ctypes as C
import os
import re
import shutil
import subprocess
import tempfile

import pytest

from mvil_fusion_amd import lib, scanreg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LLVM = "/opt/rocm/lib/llvm/bin"


def test_library_exports_every_vscan_symbol():
    so = lib.load_vilsolve()
    src = open(os.path.join(ROOT, "include", "vilscan.h")).read()
    syms = sorted(set(re.findall(r"\b(vscan_[a-z_0-9]+)\s*\(", src)))
    assert syms == ["vscan_create", "vscan_default_config", "vscan_destroy", "vscan_extract", "vscan_profile_enable", "vscan_profile_read"], syms
    for s in syms:
        assert hasattr(so, s), "libvilsolve.so does not export %s" % s


def test_struct_layouts_match_header():
    prog = '#include <stdio.h>\n#include "vilscan.h"\nint main(void){printf("%zu %zu %zu %d %d\\n", sizeof(vscan_config), sizeof(vscan_cloud), sizeof(vscan_result), VSCAN_MAX_RING_POINTS, VSCAN_NUM_KERNELS);return 0;}\n'
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "s.c"), "w").write(prog)
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), os.path.join(d, "s.c"), "-o", os.path.join(d, "s")])
        out = [int(v) for v in subprocess.check_output([os.path.join(d, "s")]).decode().split()]
    assert [C.sizeof(scanreg.VscanConfig), C.sizeof(scanreg.VscanCloud), C.sizeof(scanreg.VscanResult), scanreg.MAX_RING_POINTS, len(scanreg.KERNELS)] == out


def test_default_config_is_the_reference_one():
    cfg = scanreg.default_config(lib.load_vilsolve())
    got = (cfg.num_rings, cfg.lower_bound_deg, cfg.upper_bound_deg, cfg.num_scan_subregions, cfg.num_curvature_regions, cfg.surf_curv_th, cfg.max_corner_sharp,
           cfg.max_corner_less_sharp, cfg.max_surf_flat, round(cfg.less_flat_filter_size, 6), cfg.uneven)
    assert got == (16, -15.0, 15.0, 8, 5, 1.0, 3, 30, 4, 0.2, 0)                # PointProcessor.h:34-41, scanRegistration.cpp:17


def test_create_refuses_without_device():
    """No device (or, on a GPU machine, a device index that does not exist): VIL_ERR_DEVICE, there is no CPU fallback."""
    import torch
    with pytest.raises(scanreg.ScanRegError) as e:
        scanreg.ScanReg(lib.load_vilsolve(), device=1 << 20 if torch.cuda.is_available() else 0)
    assert e.value.status == -2


@pytest.mark.skipif(not (os.path.exists(os.path.join(LLVM, "llvm-objdump")) and os.path.exists(os.path.join(LLVM, "llvm-readelf"))), reason="needs the ROCm LLVM tools")
def test_scan_kernels_do_not_spill_vector_registers():
    """Read from the code object's notes, as test_build_no_spills.py does for the solver's kernels; k_scan_features also has to stay
    inside the 160 kB of local memory with 1024 threads (<= 128 vector registers)."""
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
    for k in scanreg.KERNELS:
        hit = [n for n in seen if k in n]
        assert len(hit) == 1, (k, sorted(seen))
        spill, scratch, vgprs, lds = seen[hit[0]]
        assert spill == 0 and scratch == 0, "%s spills %d vector registers (%d B of scratch per lane)" % (k, spill, scratch)
        assert vgprs <= 128 and lds <= 160 * 1024, (k, vgprs, lds)
    assert [v[3] for n, v in seen.items() if "k_scan_features" in n][0] > 64 * 1024      # the ring, its keys and the filter's table
