"""No-GPU checks of include/vilepi.h (epipolar outlier rejection and undistortion): libvilsolve.so exports every declared symbol, the ctypes
mirrors have the C compiler's layout, vepi_create and the calls check their arguments first and then refuse to run without a device, and
none of the row's kernels spills or uses scratch."""
import ctypes as C
import os
import re
import shutil
import subprocess
import tempfile

import numpy as np
import pytest

from mvil_fusion_amd import epipolar, lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LLVM = "/opt/rocm/lib/llvm/bin"
CAM = epipolar.REFERENCE_CAMERA


def test_library_exports_every_vepi_symbol():
    so = lib.load_vilsolve()
    src = open(os.path.join(ROOT, "include", "vilepi.h")).read()
    syms = sorted(set(re.findall(r"\b(vepi_[a-z_0-9]+)\s*\(", src)))
    assert syms == ["vepi_create", "vepi_debug_read", "vepi_destroy", "vepi_profile_enable", "vepi_profile_read", "vepi_reject", "vepi_reset", "vepi_undistort"], syms
    for s in syms:
        assert hasattr(so, s), "libvilsolve.so does not export %s" % s


def test_struct_layout_and_constants_match_header():
    cfg_f = ("fx", "fy", "cx", "cy", "k1", "k2", "p1", "p2", "focal", "width", "height", "model", "max_points", "max_iters", "batch", "readback", "reserved")
    sum_f = ("n_points", "n_inliers", "found", "best_hypothesis", "consumed", "evaluated", "launches", "reserved")
    fields = [("vepi_cfg", f) for f in cfg_f] + [("vepi_summary", f) for f in sum_f]
    structs = ["vepi_cfg", "vepi_summary"]
    consts = ["VEPI_NUM_KERNELS", "VEPI_MIN_POINTS_LIMIT", "VEPI_MAX_POINTS_LIMIT", "VEPI_MAX_ITERS_LIMIT", "VEPI_SAMPLE", "VEPI_JACOBI_SWEEPS", "VEPI_LIFT_STEPS",
              "VEPI_MODEL_PINHOLE", "VEPI_MODEL_CATA", "VEPI_MODEL_EQUIDISTANT", "VEPI_MODEL_SCARAMUZZA", "VEPI_READBACK_PINNED", "VEPI_READBACK_COPY",
              "VEPI_DBG_CUR_PTS", "VEPI_DBG_FORW_PTS", "VEPI_DBG_SAMPLES", "VEPI_DBG_COUNTS", "VEPI_DBG_F", "VEPI_DBG_MARGINS"]
    prog = ('#include <stdio.h>\n#include <stddef.h>\n#include "vilepi.h"\nint main(void){' +
            "".join('printf("%%zu ", sizeof(%s));' % s for s in structs) + "".join('printf("%%zu ", offsetof(%s, %s));' % f for f in fields) +
            "".join('printf("%%d ", (int)%s);' % c for c in consts) + "return 0;}\n")
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "s.c"), "w").write(prog)
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), os.path.join(d, "s.c"), "-o", os.path.join(d, "s")])
        out = [int(v) for v in subprocess.check_output([os.path.join(d, "s")]).decode().split()]
    e = epipolar
    mirror = {"vepi_cfg": e.VepiCfg, "vepi_summary": e.VepiSummary}
    assert [f for f, _ in e.VepiCfg._fields_] == list(cfg_f) and [f for f, _ in e.VepiSummary._fields_] == list(sum_f)
    m = e.MODELS
    assert [C.sizeof(mirror[s]) for s in structs] + [getattr(mirror[s], f).offset for s, f in fields] + \
           [len(e.KERNELS), e.MIN_POINTS_LIMIT, e.MAX_POINTS_LIMIT, e.MAX_ITERS_LIMIT, e.SAMPLE, e.JACOBI_SWEEPS, e.LIFT_STEPS, m["PINHOLE"], m["CATA"], m["EQUIDISTANT"],
            m["SCARAMUZZA"], e.READBACK_PINNED, e.READBACK_COPY, e.DBG_CUR_PTS, e.DBG_FORW_PTS, e.DBG_SAMPLES, e.DBG_COUNTS, e.DBG_F, e.DBG_MARGINS] == out
    import epipolar_ref as er
    assert (er.SAMPLE, er.SWEEPS, er.LIFT_STEPS) == (e.SAMPLE, e.JACOBI_SWEEPS, e.LIFT_STEPS)      # the restatement's constants are the header's
    assert {k: er.REFERENCE_CAMERA[k] for k in er.REFERENCE_CAMERA} == {k: CAM[k] for k in er.REFERENCE_CAMERA}


def test_header_states_the_generator_of_the_restatement():
    import epipolar_ref as er
    src = open(os.path.join(ROOT, "include", "vilepi.h")).read()
    for k in (er.HYP_MUL, er.MIX_ADD, er.MIX_M1, er.MIX_M2):
        assert "0x%016X" % k in src, hex(k)


def test_create_checks_its_arguments_first_and_refuses_without_device():
    """No device (or, on a GPU machine, a device index that does not exist): VIL_ERR_DEVICE, there is no CPU fallback.  A bad configuration
    is VIL_ERR_INVALID_ARGUMENT and another camera model VIL_ERR_UNSUPPORTED, with or without a device."""
    import torch
    so = lib.load_vilsolve()
    nodev = 1 << 20 if torch.cuda.is_available() else 0
    with pytest.raises(epipolar.EpipolarError) as e:
        epipolar.Epipolar(so, CAM, device=nodev)
    assert e.value.status == -2
    for bad in (dict(max_points=7), dict(max_points=4097), dict(max_iters=0), dict(max_iters=65537), dict(batch=-1), dict(batch=1001), dict(readback=2)):
        with pytest.raises(epipolar.EpipolarError) as e:
            epipolar.Epipolar(so, CAM, device=nodev, **bad)
        assert e.value.status == -1, bad
    for bad in (dict(fx=0.0), dict(fy=float("nan")), dict(k1=float("inf")), dict(width=0), dict(height=65537), dict(focal=float("nan"))):
        with pytest.raises(epipolar.EpipolarError) as e:
            epipolar.Epipolar(so, dict(CAM, **bad), device=nodev)
        assert e.value.status == -1, bad
    for model in ("CATA", "EQUIDISTANT", "SCARAMUZZA"):
        with pytest.raises(epipolar.EpipolarError) as e:
            epipolar.Epipolar(so, CAM, model=model, device=nodev)
        assert e.value.status == -6, model
    with pytest.raises(epipolar.EpipolarError) as e:        # the argument check comes before the model's
        epipolar.Epipolar(so, CAM, model="CATA", max_points=3, device=nodev)
    assert e.value.status == -1
    f = so.vepi_create; f.restype = C.c_int
    cfg = epipolar.VepiCfg(356.0, 355.0, 320.0, 240.0, 0, 0, 0, 0, 460.0, 640, 480, 0, 128, 100, 0, 0, 0)
    assert f(C.c_int32(nodev), C.byref(cfg), None) == -1
    assert f(C.c_int32(nodev), None, C.byref(C.c_void_p())) == -1
    cfg.model = 7
    assert f(C.c_int32(nodev), C.byref(cfg), C.byref(C.c_void_p())) == -1


def test_calls_refuse_a_null_context():
    so = lib.load_vilsolve()
    buf = np.zeros(64, np.float32)
    p = C.c_void_p(buf.ctypes.data)
    for name, args in (("vepi_reject", (None, C.c_int32(8), p, p, C.c_double(1.0), C.c_double(0.99), C.c_uint64(1), p, None)),
                       ("vepi_undistort", (None, C.c_int32(4), p, p, C.c_double(0.1), p, p)), ("vepi_reset", (None,)),
                       ("vepi_debug_read", (None, C.c_int32(0), p, C.c_int64(256))), ("vepi_profile_enable", (None, C.c_int32(1))), ("vepi_profile_read", (None, p, p))):
        f = getattr(so, name); f.restype = C.c_int
        assert f(*args) == -1, name
    assert not buf.any()
    so.vepi_destroy.restype = None
    so.vepi_destroy(None)


@pytest.mark.skipif(not (os.path.exists(os.path.join(LLVM, "llvm-objdump")) and os.path.exists(os.path.join(LLVM, "llvm-readelf"))), reason="needs the ROCm LLVM tools")
def test_epi_kernels_do_not_spill_or_use_scratch():
    """Read from the code object's notes, as test_track_abi.py does: spill 0, scratch 0.  A 9 x 9 fp64 Jacobi per lane in registers would
    spill; k_epi_hyp keeps the matrices in LDS."""
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
    assert len(epipolar.KERNELS) == 3
    for k in epipolar.KERNELS:
        hit = [n for n in seen if k in n]
        assert len(hit) == 1, (k, sorted(seen))
        vspill, sspill, scratch, vgprs, lds = seen[hit[0]]
        print(k, "vgprs", vgprs, "lds", lds)
        assert vspill == 0 and sspill == 0 and scratch == 0, "%s spills %d vector / %d scalar registers (%d B of scratch per lane)" % (k, vspill, sspill, scratch)
        assert lds <= 64 * 1024, (k, lds)
