"""No-GPU checks of include/vilclahe.h (CLAHE in front of the feature tracker): libvilsolve.so exports every declared symbol, the ctypes
mirror has the C compiler's layout, vclahe_create checks its arguments and then refuses to run without a device, and none of the row's
kernels spills, uses scratch or takes more than 160 kB of LDS."""
import ctypes as C
import os
import re
import shutil
import subprocess
import tempfile

import pytest

from mvil_fusion_amd import clahe, lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LLVM = "/opt/rocm/lib/llvm/bin"


def test_library_exports_every_vclahe_symbol():
    so = lib.load_vilsolve()
    src = open(os.path.join(ROOT, "include", "vilclahe.h")).read()
    syms = sorted(set(re.findall(r"\b(vclahe_[a-z_0-9]+)\s*\(", src)))
    assert syms == ["vclahe_apply", "vclahe_create", "vclahe_debug_read", "vclahe_destroy", "vclahe_profile_enable", "vclahe_profile_read", "vclahe_push"], syms
    for s in syms:
        assert hasattr(so, s), "libvilsolve.so does not export %s" % s


def test_the_tracker_stages_are_not_exported():
    """vclahe_push reaches the tracker through csrc/viltrack_stage.hpp: hidden C++ symbols, no new vtrack_* entry point."""
    out = subprocess.run(["nm", "-D", "--defined-only", lib.LIB_PATH], check=True, capture_output=True, text=True).stdout
    names = [l.split()[-1] for l in out.splitlines() if l.strip()]
    assert sorted(n for n in names if n.startswith("vtrack_")) == ["vtrack_create", "vtrack_debug_read", "vtrack_destroy", "vtrack_detect", "vtrack_profile_enable",
                                                                  "vtrack_profile_read", "vtrack_push_image", "vtrack_track"]
    assert not [n for n in names if "viltrack_stage" in n], "the stage functions are exported"


def test_struct_layout_and_constants_match_header():
    fields = [("vclahe_cfg", f) for f in ("width", "height", "tiles_x", "tiles_y", "clip_limit")]
    consts = ["VCLAHE_NUM_KERNELS", "VCLAHE_MAX_TILES", "VCLAHE_DBG_HIST", "VCLAHE_DBG_LUT"]
    prog = ('#include <stdio.h>\n#include <stddef.h>\n#include "vilclahe.h"\nint main(void){printf("%zu ", sizeof(vclahe_cfg));' +
            "".join('printf("%%zu ", offsetof(%s, %s));' % f for f in fields) + "".join('printf("%%d ", (int)%s);' % c for c in consts) + "return 0;}\n")
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "s.c"), "w").write(prog)
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), os.path.join(d, "s.c"), "-o", os.path.join(d, "s")])
        out = [int(v) for v in subprocess.check_output([os.path.join(d, "s")]).decode().split()]
    assert [C.sizeof(clahe.VclaheCfg)] + [getattr(clahe.VclaheCfg, f).offset for _, f in fields] + [len(clahe.KERNELS), clahe.MAX_TILES, clahe.DBG_HIST, clahe.DBG_LUT] == out
    assert out[0] == 24 and out[5] == 16


def test_create_checks_its_arguments_first_and_refuses_without_device():
    """No device (or, on a GPU machine, a device index that does not exist): VIL_ERR_DEVICE, there is no CPU fallback.  A bad
    configuration is VIL_ERR_INVALID_ARGUMENT with or without a device."""
    import torch
    so = lib.load_vilsolve()
    nodev = 1 << 20 if torch.cuda.is_available() else 0
    good = dict(width=128, height=96, tiles_x=8, tiles_y=8, clip_limit=3.0)
    for ok in (good, dict(good, clip_limit=0.0), dict(good, tiles_x=1, tiles_y=16), dict(good, width=16, height=16384)):
        with pytest.raises(clahe.ClaheError) as e:
            clahe.Clahe(so, device=nodev, **ok)
        assert e.value.status == -2, ok
    for bad in (dict(width=15), dict(height=0), dict(width=16385), dict(height=16385), dict(tiles_x=0), dict(tiles_x=17), dict(tiles_y=0), dict(tiles_y=17), dict(tiles_y=-1),
                dict(clip_limit=-0.5), dict(clip_limit=float("nan")), dict(clip_limit=float("inf"))):
        with pytest.raises(clahe.ClaheError) as e:
            clahe.Clahe(so, device=nodev, **dict(good, **bad))
        assert e.value.status == -1, bad
    f = so.vclahe_create; f.restype = C.c_int
    cfg = clahe.VclaheCfg(128, 96, 8, 8, 3.0)
    assert f(C.c_int32(nodev), C.byref(cfg), None) == -1
    assert f(C.c_int32(nodev), None, C.byref(C.c_void_p())) == -1
    for name, args in (("vclahe_apply", (None, None, 0, None, 0)), ("vclahe_push", (None, None, None, 0, None, 0)), ("vclahe_debug_read", (None, 0, None, C.c_int64(0))),
                       ("vclahe_profile_enable", (None, 1)), ("vclahe_profile_read", (None, None, None))):
        g = getattr(so, name); g.restype = C.c_int
        assert g(*args) == -1, name                         # a NULL context


@pytest.mark.skipif(not (os.path.exists(os.path.join(LLVM, "llvm-objdump")) and os.path.exists(os.path.join(LLVM, "llvm-readelf"))), reason="needs the ROCm LLVM tools")
def test_clahe_kernels_do_not_spill_or_use_scratch():
    """Read from the code object's notes, as test_track_abi.py does: spill 0, scratch 0, <= 160 kB of LDS."""
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
                s = re.search(r"\.sgpr_spill_count:\s*(\d+)", blk); v = re.search(r"\.vgpr_count:\s*(\d+)", blk); g = re.findall(r"\.group_segment_fixed_size:\s*(\d+)", before)
                if m and p and s and v and g: seen[name] = (int(m.group(1)), int(s.group(1)), int(p.group(1)), int(v.group(1)), int(g[-1]))
    assert len(clahe.KERNELS) == 3
    for k in clahe.KERNELS:
        hit = [n for n in seen if k in n]
        assert len(hit) == 1, (k, sorted(seen))
        vspill, sspill, scratch, vgprs, lds = seen[hit[0]]
        print(k, "vgprs", vgprs, "lds", lds)
        assert vspill == 0 and sspill == 0 and scratch == 0, "%s spills %d vector / %d scalar registers (%d B of scratch per lane)" % (k, vspill, sspill, scratch)
        assert lds <= 160 * 1024, (k, lds)
