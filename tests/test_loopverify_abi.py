"""No-GPU checks of include/villoop.h (alignment fitness score and loop-closure verification): libvilsolve.so exports every declared
symbol, the ctypes mirrors have the C compiler's layout, vloop_create checks its arguments and then refuses to run without a device, and
none of the row's kernels spills vector registers."""
import ctypes as C
import os
import re
import shutil
import subprocess
import tempfile

import pytest

from mvil_fusion_amd import lib, loopverify

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LLVM = "/opt/rocm/lib/llvm/bin"


def test_library_exports_every_vloop_symbol():
    so = lib.load_vilsolve()
    src = open(os.path.join(ROOT, "include", "villoop.h")).read()
    syms = sorted(set(re.findall(r"\b(vloop_[a-z_0-9]+)\s*\(", src)))
    assert syms == ["vloop_create", "vloop_default_options", "vloop_destroy", "vloop_profile_enable", "vloop_profile_read", "vloop_score", "vloop_set_grid", "vloop_set_source",
                    "vloop_set_target", "vloop_verify"], syms
    for s in syms:
        assert hasattr(so, s), "libvilsolve.so does not export %s" % s


def test_struct_layout_constants_and_defaults_match_header():
    fields = [("vloop_candidate", "xyz"), ("vloop_candidate", "guess"), ("vloop_options", "resolution"), ("vloop_options", "max_tolerable_fitness"),
              ("vloop_candidate_result", "iterations"), ("vloop_candidate_result", "T"), ("vloop_best", "n_used"), ("vloop_best", "T"), ("vloop_best", "delta")]
    structs = ["vloop_candidate", "vloop_options", "vloop_candidate_result", "vloop_best"]
    prog = ('#include <stdio.h>\n#include <stddef.h>\n#include "villoop.h"\nint main(void){' +
            "".join('printf("%%zu ", sizeof(%s));' % s for s in structs) + "".join('printf("%%zu ", offsetof(%s, %s));' % f for f in fields) +
            'printf("%d %d %d\\n", VLOOP_NUM_KERNELS, VLOOP_MAX_BATCH, VLOOP_SUM_BLOCK);return 0;}\n')
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "s.c"), "w").write(prog)
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), os.path.join(d, "s.c"), "-o", os.path.join(d, "s")])
        out = [int(v) for v in subprocess.check_output([os.path.join(d, "s")]).decode().split()]
    lv = loopverify
    mirror = {"vloop_candidate": lv.VloopCandidate, "vloop_options": lv.VloopOptions, "vloop_candidate_result": lv.VloopCandidateResult, "vloop_best": lv.VloopBest}
    assert [C.sizeof(mirror[s]) for s in structs] + [getattr(mirror[s], f).offset for s, f in fields] + [len(lv.KERNELS), lv.MAX_BATCH, lv.SUM_BLOCK] == out
    o = lv.default_options(lib.load_vilsolve())
    assert (o.resolution, o.max_tolerable_fitness, o.reg.max_iterations, o.reg.neighbor_mode) == (0.5, 1.0, 64, 1)


def test_create_checks_its_arguments_first_and_refuses_without_device():
    """No device (or, on a GPU machine, a device index that does not exist): VIL_ERR_DEVICE, there is no CPU fallback.  A size that is
    not positive is VIL_ERR_INVALID_ARGUMENT with or without a device."""
    import torch
    so = lib.load_vilsolve()
    nodev = 1 << 20 if torch.cuda.is_available() else 0
    with pytest.raises(loopverify.LoopVerifyError) as e:
        loopverify.LoopVerify(so, device=nodev)
    assert e.value.status == -2
    for n in (0, -5):
        with pytest.raises(loopverify.LoopVerifyError) as e:
            loopverify.LoopVerify(so, max_points=n, device=nodev)
        assert e.value.status == -1, n
    f = so.vloop_create; f.restype = C.c_int
    assert f(C.c_int32(nodev), C.c_int32(16), None) == -1


@pytest.mark.skipif(not (os.path.exists(os.path.join(LLVM, "llvm-objdump")) and os.path.exists(os.path.join(LLVM, "llvm-readelf"))), reason="needs the ROCm LLVM tools")
def test_loopverify_kernels_do_not_spill_vector_registers():
    """Read from the code object's notes, as test_scancontext_abi.py does: no spill, no scratch, <= 128 vector registers, <= 160 kB of LDS."""
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
    for k in loopverify.KERNELS:
        hit = [n for n in seen if k in n]
        assert len(hit) == 1, (k, sorted(seen))
        spill, scratch, vgprs, lds = seen[hit[0]]
        print(k, "vgprs", vgprs, "lds", lds)
        assert spill == 0 and scratch == 0, "%s spills %d vector registers (%d B of scratch per lane)" % (k, spill, scratch)
        assert vgprs <= 128 and lds <= 160 * 1024, (k, vgprs, lds)
