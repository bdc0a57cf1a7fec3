"""No-GPU checks of include/vilsc.h (Scan Context place recognition): libvilsolve.so exports every declared symbol, the ctypes mirror has
the C compiler's layout, vsc_create refuses to run without a device, and none of the new kernels spills vector registers."""
import ctypes as C
import os
import re
import shutil
import subprocess
import tempfile

import pytest

from mvil_fusion_amd import lib, scancontext

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LLVM = "/opt/rocm/lib/llvm/bin"


def test_library_exports_every_vsc_symbol():
    so = lib.load_vilsolve()
    src = open(os.path.join(ROOT, "include", "vilsc.h")).read()
    syms = sorted(set(re.findall(r"\b(vsc_[a-z_0-9]+)\s*\(", src)))
    assert syms == ["vsc_count", "vsc_create", "vsc_debug_read", "vsc_default_config", "vsc_destroy", "vsc_detect", "vsc_profile_enable", "vsc_profile_read", "vsc_push_descriptor",
                    "vsc_push_scan", "vsc_read_entry", "vsc_reset"], syms
    for s in syms:
        assert hasattr(so, s), "libvilsolve.so does not export %s" % s


def test_struct_layout_constants_and_defaults_match_header():
    prog = ('#include <stdio.h>\n#include <stddef.h>\n#include "vilsc.h"\nint main(void){printf("%zu %zu %zu %zu %zu %d %d %d %d %d %d\\n", sizeof(vsc_config), sizeof(vsc_result), '
            'offsetof(vsc_config, num_exclude_recent), offsetof(vsc_result, loop_id), offsetof(vsc_result, yaw_diff_rad), VSC_NUM_RING, VSC_NUM_SECTOR, VSC_MAX_CANDIDATES, '
            'VSC_NUM_KERNELS, VSC_MODE_REFERENCE, VSC_MODE_EXHAUSTIVE);return 0;}\n')
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "s.c"), "w").write(prog)
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), os.path.join(d, "s.c"), "-o", os.path.join(d, "s")])
        out = [int(v) for v in subprocess.check_output([os.path.join(d, "s")]).decode().split()]
    sc = scancontext
    assert [C.sizeof(sc.VscConfig), C.sizeof(sc.VscResult), sc.VscConfig.num_exclude_recent.offset, sc.VscResult.loop_id.offset, sc.VscResult.yaw_diff_rad.offset, sc.NUM_RING,
            sc.NUM_SECTOR, sc.MAX_CANDIDATES, len(sc.KERNELS), sc.MODE_REFERENCE, sc.MODE_EXHAUSTIVE] == out
    cfg = sc.default_config(lib.load_vilsolve())
    assert (cfg.lidar_height, cfg.max_radius, cfg.dist_thres, cfg.search_ratio, cfg.num_exclude_recent, cfg.num_candidates) == (2.0, 80.0, 0.5, 0.1, 5, 3)


def test_create_refuses_without_device_and_checks_its_arguments_first():
    """No device (or, on a GPU machine, a device index that does not exist): VIL_ERR_DEVICE, there is no CPU fallback.  Sizes and
    configurations outside the header's ranges are VIL_ERR_INVALID_ARGUMENT with or without a device."""
    import torch
    so = lib.load_vilsolve()
    nodev = 1 << 20 if torch.cuda.is_available() else 0
    with pytest.raises(scancontext.ScanContextError) as e:
        scancontext.ScanContext(so, device=nodev)
    assert e.value.status == -2
    for kw in (dict(max_entries=0), dict(max_points=0), dict(num_candidates=17), dict(num_candidates=0), dict(max_radius=0.0), dict(search_ratio=1.5), dict(num_exclude_recent=-1)):
        with pytest.raises(scancontext.ScanContextError) as e:
            scancontext.ScanContext(so, device=nodev, **kw)
        assert e.value.status == -1, kw


@pytest.mark.skipif(not (os.path.exists(os.path.join(LLVM, "llvm-objdump")) and os.path.exists(os.path.join(LLVM, "llvm-readelf"))), reason="needs the ROCm LLVM tools")
def test_scancontext_kernels_do_not_spill_vector_registers():
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
    for k in scancontext.KERNELS:
        hit = [n for n in seen if k in n]
        assert len(hit) == 1, (k, sorted(seen))
        spill, scratch, vgprs, lds = seen[hit[0]]
        print(k, "vgprs", vgprs, "lds", lds)
        assert spill == 0 and scratch == 0, "%s spills %d vector registers (%d B of scratch per lane)" % (k, spill, scratch)
        assert vgprs <= 128 and lds <= 160 * 1024, (k, vgprs, lds)
