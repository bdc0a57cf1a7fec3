"""No-GPU checks of include/vilfeat.h (the device-resident feature tracker): libvilsolve.so exports every declared symbol, the ctypes mirrors
have the C compiler's layout, vfeat_create checks its arguments, then the camera model, and then refuses to run without a device, and
none of the row's new kernels spills, uses scratch or takes more than 160 kB of LDS."""
import ctypes as C
import os
import re
import shutil
import subprocess
import tempfile

import pytest

import feat_ref as fr
from mvil_fusion_amd import feat, lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LLVM = "/opt/rocm/lib/llvm/bin"
SMALL = dict(width=128, height=96, camera=fr.camera(128, 96), max_level=1, max_points=64, max_candidates=4096, max_iters=64, max_cnt=40, min_dist=10)


def test_library_exports_every_vfeat_symbol():
    so = lib.load_vilsolve()
    src = open(os.path.join(ROOT, "include", "vilfeat.h")).read()
    syms = sorted(set(re.findall(r"\b(vfeat_[a-z_0-9]+)\s*\(", src)))
    assert syms == ["vfeat_create", "vfeat_debug_read", "vfeat_destroy", "vfeat_profile_enable", "vfeat_profile_read", "vfeat_read_image", "vfeat_reset"], syms
    for s in syms:
        assert hasattr(so, s), "libvilsolve.so does not export %s" % s


def test_struct_layout_and_constants_match_header():
    mirror = {"vfeat_cfg": feat.VfeatCfg, "vfeat_msg": feat.VfeatMsg, "vfeat_summary": feat.VfeatSummary}
    structs = list(mirror)
    fields = [(s, f) for s in structs for f, _ in mirror[s]._fields_]
    consts = ["VFEAT_NUM_KERNELS", "VFEAT_MIN_POINTS_LIMIT", "VFEAT_MAX_POINTS_LIMIT", "VFEAT_HEADER_BYTES", "VFEAT_ROW_BYTES", "VFEAT_DBG_STATE", "VFEAT_DBG_UN_VEL",
              "VFEAT_DBG_CUR_LEVEL", "VFEAT_DBG_FORW_LEVEL"]
    prog = ('#include <stdio.h>\n#include <stddef.h>\n#include "vilfeat.h"\nint main(void){' +
            "".join('printf("%%zu ", sizeof(%s));' % s for s in structs) + "".join('printf("%%zu ", offsetof(%s, %s));' % f for f in fields) +
            "".join('printf("%%d ", (int)%s);' % c for c in consts) + "return 0;}\n")
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "s.c"), "w").write(prog)
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), os.path.join(d, "s.c"), "-o", os.path.join(d, "s")])
        out = [int(v) for v in subprocess.check_output([os.path.join(d, "s")]).decode().split()]
    f = feat
    assert [C.sizeof(mirror[s]) for s in structs] + [getattr(mirror[s], fld).offset for s, fld in fields] + \
           [len(f.KERNELS), f.MIN_POINTS_LIMIT, f.MAX_POINTS_LIMIT, f.HEADER_BYTES, f.ROW_BYTES, f.DBG_STATE, f.DBG_UN_VEL, f.DBG_CUR_LEVEL, f.DBG_FORW_LEVEL] == out
    assert f.ROW_BYTES == 4 * (3 + 5)                       # points_xyz and the five channels, float32


def test_create_checks_its_arguments_then_the_model_then_the_device():
    """One bad value per field: VIL_ERR_INVALID_ARGUMENT with or without a device.  Another model than PINHOLE: VIL_ERR_UNSUPPORTED.  No
    device (or, on a GPU machine, a device index that does not exist): VIL_ERR_DEVICE, there is no CPU fallback."""
    import torch
    so = lib.load_vilsolve()
    nodev = 1 << 20 if torch.cuda.is_available() else 0
    with pytest.raises(feat.FeatError) as e:
        feat.FeatureTracker(so, device=nodev, **SMALL)
    assert e.value.status == -2
    nan, inf = float("nan"), float("inf")
    cam = SMALL["camera"]
    bads = [dict(width=15), dict(width=16385), dict(height=15), dict(height=16385), dict(max_level=-1), dict(max_level=4), dict(max_points=7), dict(max_points=4097),
            dict(max_candidates=0), dict(max_iters=0), dict(max_iters=65537), dict(equalize=2), dict(equalize=True, tiles_x=0), dict(equalize=True, tiles_x=17),
            dict(equalize=True, tiles_y=0), dict(equalize=True, tiles_y=17), dict(equalize=True, clip_limit=-1.0), dict(equalize=True, clip_limit=nan), dict(max_cnt=0),
            dict(max_cnt=65), dict(min_dist=-1), dict(min_dist=1025), dict(quality=0.0), dict(quality=1.5), dict(quality=nan), dict(f_threshold=0.0), dict(f_threshold=inf),
            dict(f_threshold=nan), dict(confidence=0.0), dict(confidence=1.0), dict(confidence=nan), dict(camera=dict(cam, fx=0.0)), dict(camera=dict(cam, fy=0.0))] + \
           [dict(camera=dict(cam, **{k: nan})) for k in ("fx", "fy", "cx", "cy", "k1", "k2", "p1", "p2", "focal")]
    for bad in bads:
        with pytest.raises(feat.FeatError) as e:
            feat.FeatureTracker(so, device=nodev, **dict(SMALL, **bad))
        assert e.value.status == -1, bad
    with pytest.raises(feat.FeatError) as e:                # a bad value is reported before the model
        feat.FeatureTracker(so, device=nodev, **dict(SMALL, model="CATA", max_cnt=0))
    assert e.value.status == -1
    for model in ("CATA", "EQUIDISTANT", "SCARAMUZZA"):
        with pytest.raises(feat.FeatError) as e:
            feat.FeatureTracker(so, device=nodev, **dict(SMALL, model=model))
        assert e.value.status == -6, model
    with pytest.raises(feat.FeatError) as e:
        feat.FeatureTracker(so, device=nodev, **dict(SMALL, tiles_x=0, clip_limit=-1.0))
    assert e.value.status == -2
    f = so.vfeat_create; f.restype = C.c_int
    cfg = feat.VfeatCfg()
    assert f(C.c_int32(nodev), C.byref(cfg), None) == -1
    assert f(C.c_int32(nodev), None, C.byref(C.c_void_p())) == -1
    for name in ("vfeat_reset", "vfeat_profile_enable"):
        g = getattr(so, name); g.restype = C.c_int
        assert g(None, C.c_int32(0)) == -1
    g = so.vfeat_read_image; g.restype = C.c_int
    assert g(None, None, C.c_int32(0), C.c_double(0.0), C.c_int32(0), C.c_uint64(0), None, None) == -1


@pytest.mark.skipif(not (os.path.exists(os.path.join(LLVM, "llvm-objdump")) and os.path.exists(os.path.join(LLVM, "llvm-readelf"))), reason="needs the ROCm LLVM tools")
def test_feat_kernels_do_not_spill_or_use_scratch():
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
    assert len(feat.KERNELS) == 5
    for k in feat.KERNELS:
        hit = [n for n in seen if k in n]
        assert len(hit) == 1, (k, sorted(seen))
        vspill, sspill, scratch, vgprs, lds = seen[hit[0]]
        print(k, "vgprs", vgprs, "lds", lds)
        assert vspill == 0 and sspill == 0 and scratch == 0, "%s spills %d vector / %d scalar registers (%d B of scratch per lane)" % (k, vspill, sspill, scratch)
        assert lds <= 160 * 1024, (k, lds)
