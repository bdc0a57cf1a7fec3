"""No-GPU checks of include/villmap.h (the resident local cube map): libvilsolve.so exports every declared symbol and nothing of the stage
headers it is built on, the vmap_* export list is what it was, the ctypes mirrors have the C compiler's layout and the header's
defaults, vlmap_create refuses to run without a device, and none of the new kernels spills vector registers."""
import ctypes as C
import os
import re
import shutil
import subprocess
import tempfile

import pytest

from mvil_fusion_amd import lib, localmap, mapreg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LLVM = "/opt/rocm/lib/llvm/bin"
SYMS = ["vlmap_create", "vlmap_debug_read", "vlmap_debug_write_cube", "vlmap_default_config", "vlmap_destroy", "vlmap_profile_enable", "vlmap_profile_read", "vlmap_push_scan", "vlmap_read_cube",
        "vlmap_read_published", "vlmap_reset"]


def exported():
    out = subprocess.run(["nm", "-D", "--defined-only", lib.LIB_PATH], check=True, capture_output=True, text=True).stdout
    return [l.split()[-1] for l in out.splitlines() if l.strip()]


def test_library_exports_every_vlmap_symbol():
    so = lib.load_vilsolve()
    src = open(os.path.join(ROOT, "include", "villmap.h")).read()
    syms = sorted(set(re.findall(r"\b(vlmap_[a-z_0-9]+)\s*\(", src)))
    assert syms == SYMS, syms
    for s in syms:
        assert hasattr(so, s), "libvilsolve.so does not export %s" % s
    assert sorted(n for n in exported() if "vlmap" in n) == SYMS


def test_no_stage_symbol_is_exported_and_vmap_is_unchanged():
    names = exported()
    assert not [n for n in names if "vilmap_stage" in n or "vilcloud_stage" in n or "vilcloud_dev" in n], "stage functions are exported"
    assert sorted(n for n in names if n.startswith("vmap_")) == ["vmap_align", "vmap_associate", "vmap_create", "vmap_destroy", "vmap_profile_enable", "vmap_profile_read",
                                                                 "vmap_set_fused_max", "vmap_set_map"]
    # the sets the other rows' ABI tests list exactly are not added to
    mine = [n for n in names if "lmap" in n]
    assert not [n for n in mine if "vcloud" in n or "vfront" in n or n.startswith("vdepth_") or n.startswith("vtrack_")], mine


def test_struct_layout_constants_and_defaults_match_header():
    fields = [("vlmap_config", f) for f, _ in localmap.VlmapConfig._fields_] + [("vlmap_summary", f) for f, _ in localmap.VlmapSummary._fields_]
    consts = ["VLMAP_W", "VLMAP_H", "VLMAP_D", "VLMAP_CUBES", "VLMAP_MAX_VALID", "VLMAP_NUM_KERNELS", "VLMAP_DBG_CORNER_STACK", "VLMAP_DBG_SURF_STACK", "VLMAP_DBG_CORNER_FROM_MAP",
              "VLMAP_DBG_SURF_FROM_MAP", "VLMAP_DBG_MATRIX", "VLMAP_FRAME_WORLD", "VLMAP_FRAME_SENSOR", "VIL_ERR_INVALID_ARGUMENT", "VIL_ERR_DEVICE", "VIL_ERR_CAPACITY"]
    prog = ('#include <stdio.h>\n#include <stddef.h>\n#include "villmap.h"\nint main(void){printf("%zu %zu %zu ", sizeof(vlmap_config), sizeof(vlmap_summary), sizeof(vmap_summary));' +
            "".join('printf("%%zu ", offsetof(%s, %s));' % sf for sf in fields) + "".join('printf("%%d ", (int)%s);' % c for c in consts) + 'printf("\\n");return 0;}\n')
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "s.c"), "w").write(prog)
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), os.path.join(d, "s.c"), "-o", os.path.join(d, "s")])
        out = [int(v) for v in subprocess.check_output([os.path.join(d, "s")]).decode().split()]
    mine = [C.sizeof(localmap.VlmapConfig), C.sizeof(localmap.VlmapSummary), C.sizeof(mapreg.VmapSummary)]
    mine += [getattr(localmap.VlmapConfig, f).offset for f, _ in localmap.VlmapConfig._fields_] + [getattr(localmap.VlmapSummary, f).offset for f, _ in localmap.VlmapSummary._fields_]
    mine += [localmap.W, localmap.H, localmap.D, localmap.CUBES, localmap.MAX_VALID, len(localmap.KERNELS), localmap.DBG_CORNER_STACK, localmap.DBG_SURF_STACK,
             localmap.DBG_CORNER_FROM_MAP, localmap.DBG_SURF_FROM_MAP, localmap.DBG_MATRIX, localmap.FRAME_WORLD, localmap.FRAME_SENSOR, localmap.ERR_INVALID_ARGUMENT,
             localmap.ERR_DEVICE, localmap.ERR_CAPACITY]
    assert mine == out
    g = localmap.default_config(lib.load_vilsolve())        # runs without a device
    assert (g.line_res, g.plane_res, g.hist_size, g.publish_first_frame, g.cube_length, g.cube_height, g.publish_distance, g.publish_frames, g.max_scan_points, g.max_map_points) == \
        (C.c_float(0.2).value, C.c_float(0.4).value, 512, 10, 10.0, 5.0, 2.0, 30, 1 << 15, 1 << 19)
    assert localmap.default_config(lib.load_vilsolve(), hist_size=64).hist_size == 64


def test_create_refuses_without_device():
    """No device (or, on a GPU machine, a device index that does not exist): VIL_ERR_DEVICE, there is no CPU fallback."""
    import torch
    with pytest.raises(localmap.LocalMapError) as e:
        localmap.LocalMap(lib.load_vilsolve(), device=1 << 20 if torch.cuda.is_available() else 0, max_scan_points=64, max_map_points=256)
    assert e.value.status == localmap.ERR_DEVICE
    for bad in (dict(max_scan_points=0), dict(max_map_points=32), dict(max_map_points=(1 << 24) + 1), dict(hist_size=3), dict(line_res=0.0), dict(plane_res=float("nan")),
                dict(cube_length=0.0), dict(cube_height=float("inf")), dict(publish_distance=-1.0)):
        with pytest.raises(localmap.LocalMapError) as e:
            localmap.LocalMap(lib.load_vilsolve(), **{**dict(max_scan_points=64, max_map_points=256), **bad})
        assert e.value.status == localmap.ERR_INVALID_ARGUMENT, bad


@pytest.mark.skipif(not (os.path.exists(os.path.join(LLVM, "llvm-objdump")) and os.path.exists(os.path.join(LLVM, "llvm-readelf"))), reason="needs the ROCm LLVM tools")
def test_localmap_kernels_do_not_spill_vector_registers():
    """Read from the code object's notes, as test_cloud_abi.py does: no spill, no scratch, <= 128 vector registers, <= 64 kB of LDS (the
    limit of one workgroup)."""
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
    for k in localmap.KERNELS:
        hit = [n for n in seen if k in n]
        assert len(hit) == 1, (k, sorted(seen))
        spill, scratch, vgprs, lds = seen[hit[0]]
        print(k, "vgprs", vgprs, "lds", lds)
        assert spill == 0 and scratch == 0, "%s spills %d vector registers (%d B of scratch per lane)" % (k, spill, scratch)
        assert vgprs <= 128 and lds <= 64 * 1024, (k, vgprs, lds)
