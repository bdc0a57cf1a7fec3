"""No-GPU checks of include/viltrack.h (the KLT visual front end): libvilsolve.so exports every declared symbol, the ctypes mirrors have
the C compiler's layout, vtrack_create checks its arguments and then refuses to run without a device, and none of the row's kernels
spills, uses scratch or takes more than 160 kB of LDS."""
import ctypes as C
import os
import re
import shutil
import subprocess
import tempfile

import pytest

from mvil_fusion_amd import lib, track

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LLVM = "/opt/rocm/lib/llvm/bin"


def test_library_exports_every_vtrack_symbol():
    so = lib.load_vilsolve()
    src = open(os.path.join(ROOT, "include", "viltrack.h")).read()
    syms = sorted(set(re.findall(r"\b(vtrack_[a-z_0-9]+)\s*\(", src)))
    assert syms == ["vtrack_create", "vtrack_debug_read", "vtrack_destroy", "vtrack_detect", "vtrack_profile_enable", "vtrack_profile_read", "vtrack_push_image",
                    "vtrack_track"], syms
    for s in syms:
        assert hasattr(so, s), "libvilsolve.so does not export %s" % s


def test_struct_layout_and_constants_match_header():
    fields = [("vtrack_cfg", f) for f in ("width", "height", "max_level", "max_points", "max_candidates")] + \
             [("vtrack_summary", f) for f in ("n_points", "n_tracked", "n_tracks", "n_kept", "n_candidates", "n_picked", "n_new", "rounds")]
    structs = ["vtrack_cfg", "vtrack_summary"]
    consts = ["VTRACK_NUM_KERNELS", "VTRACK_MAX_LEVEL", "VTRACK_MAX_POINTS_LIMIT", "VTRACK_MAX_MIN_DIST", "VTRACK_CODE_SKIP", "VTRACK_CODE_LOWEIG", "VTRACK_CODE_EPS", "VTRACK_CODE_OSC",
              "VTRACK_CODE_CAP", "VTRACK_CODE_OOB", "VTRACK_DBG_CUR_LEVEL", "VTRACK_DBG_FORW_LEVEL", "VTRACK_DBG_LK_CODES", "VTRACK_DBG_LK_ITERS", "VTRACK_DBG_EIG", "VTRACK_DBG_MASK",
              "VTRACK_DBG_N_CANDIDATES"]
    prog = ('#include <stdio.h>\n#include <stddef.h>\n#include "viltrack.h"\nint main(void){' +
            "".join('printf("%%zu ", sizeof(%s));' % s for s in structs) + "".join('printf("%%zu ", offsetof(%s, %s));' % f for f in fields) +
            "".join('printf("%%d ", (int)%s);' % c for c in consts) + "return 0;}\n")
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "s.c"), "w").write(prog)
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), os.path.join(d, "s.c"), "-o", os.path.join(d, "s")])
        out = [int(v) for v in subprocess.check_output([os.path.join(d, "s")]).decode().split()]
    t = track
    mirror = {"vtrack_cfg": t.VtrackCfg, "vtrack_summary": t.VtrackSummary}
    codes = t.CODES
    assert [C.sizeof(mirror[s]) for s in structs] + [getattr(mirror[s], f).offset for s, f in fields] + \
           [len(t.KERNELS), t.MAX_LEVEL, t.MAX_POINTS_LIMIT, t.MAX_MIN_DIST, codes["SKIP"], codes["LOWEIG"], codes["EPS"], codes["OSC"], codes["CAP"], codes["OOB"],
            t.DBG_CUR_LEVEL, t.DBG_FORW_LEVEL, t.DBG_LK_CODES, t.DBG_LK_ITERS, t.DBG_EIG, t.DBG_MASK, t.DBG_N_CANDIDATES] == out
    import track_ref as tr
    assert {k: getattr(tr, k) for k in codes} == codes      # the restatement numbers the codes as the header does


def test_create_checks_its_arguments_first_and_refuses_without_device():
    """No device (or, on a GPU machine, a device index that does not exist): VIL_ERR_DEVICE, there is no CPU fallback.  A bad
    configuration is VIL_ERR_INVALID_ARGUMENT with or without a device."""
    import torch
    so = lib.load_vilsolve()
    nodev = 1 << 20 if torch.cuda.is_available() else 0
    small = dict(width=128, height=96, max_level=1, max_points=128, max_candidates=4096)
    with pytest.raises(track.TrackError) as e:
        track.Tracker(so, device=nodev, **small)
    assert e.value.status == -2
    for bad in (dict(width=15), dict(height=0), dict(width=16385), dict(max_level=-1), dict(max_level=4), dict(max_points=0), dict(max_points=4097), dict(max_candidates=0)):
        with pytest.raises(track.TrackError) as e:
            track.Tracker(so, device=nodev, **dict(small, **bad))
        assert e.value.status == -1, bad
    f = so.vtrack_create; f.restype = C.c_int
    cfg = track.VtrackCfg(128, 96, 1, 128, 4096)
    assert f(C.c_int32(nodev), C.byref(cfg), None) == -1
    assert f(C.c_int32(nodev), None, C.byref(C.c_void_p())) == -1


@pytest.mark.skipif(not (os.path.exists(os.path.join(LLVM, "llvm-objdump")) and os.path.exists(os.path.join(LLVM, "llvm-readelf"))), reason="needs the ROCm LLVM tools")
def test_track_kernels_do_not_spill_or_use_scratch():
    """Read from the code object's notes, as test_globalmap_abi.py does: spill 0, scratch 0, <= 160 kB of LDS."""
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
    assert len(track.KERNELS) == 8
    for k in track.KERNELS:
        hit = [n for n in seen if k in n]
        assert len(hit) == 1, (k, sorted(seen))
        vspill, sspill, scratch, vgprs, lds = seen[hit[0]]
        print(k, "vgprs", vgprs, "lds", lds)
        assert vspill == 0 and sspill == 0 and scratch == 0, "%s spills %d vector / %d scalar registers (%d B of scratch per lane)" % (k, vspill, sspill, scratch)
        assert lds <= 160 * 1024, (k, lds)
