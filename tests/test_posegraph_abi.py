"""No-GPU checks of include/vilpgo.h (pose-graph optimisation): libvilsolve.so exports every declared symbol, the ctypes mirrors have the C
compiler's layout, the defaults and constants match the header, vpgo_create checks its arguments and then refuses to run without a device,
and none of the row's kernels spills vector registers."""
import ctypes as C
import os
import re
import shutil
import subprocess
import tempfile

import pytest

import posegraph_ref
from mvil_fusion_amd import lib, posegraph

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LLVM = "/opt/rocm/lib/llvm/bin"


def test_library_exports_every_vpgo_symbol():
    so = lib.load_vilsolve()
    src = open(os.path.join(ROOT, "include", "vilpgo.h")).read()
    syms = sorted(set(re.findall(r"\b(vpgo_[a-z_0-9]+)\s*\(", src)))
    assert syms == ["vpgo_add_between", "vpgo_add_pose", "vpgo_add_position", "vpgo_add_prior", "vpgo_create", "vpgo_default_options", "vpgo_destroy", "vpgo_eval",
                    "vpgo_get_poses", "vpgo_get_step", "vpgo_optimize", "vpgo_profile_enable", "vpgo_profile_read", "vpgo_relative", "vpgo_size"], syms
    for s in syms:
        assert hasattr(so, s), "libvilsolve.so does not export %s" % s


def test_struct_layout_constants_and_defaults_match_header():
    fields = [("vpgo_options", "initial_lambda"), ("vpgo_options", "cost_tolerance"), ("vpgo_summary", "termination"), ("vpgo_summary", "n_segments"),
              ("vpgo_summary", "initial_cost"), ("vpgo_summary", "final_lambda")]
    structs = ["vpgo_options", "vpgo_summary"]
    consts = ["VPGO_NUM_KERNELS", "VPGO_SEGMENT", "VPGO_MAX_SEPARATORS", "VPGO_SUM_BLOCK", "VPGO_MAX_ITERATIONS", "VPGO_PRIOR", "VPGO_BETWEEN", "VPGO_POSITION",
              "VPGO_TERM_NONE", "VPGO_TERM_STEP", "VPGO_TERM_COST", "VPGO_TERM_MAX_ITERATIONS", "VIL_ERR_CAPACITY"]
    prog = ('#include <stdio.h>\n#include <stddef.h>\n#include "vilpgo.h"\nint main(void){' +
            "".join('printf("%%zu ", sizeof(%s));' % s for s in structs) + "".join('printf("%%zu ", offsetof(%s, %s));' % f for f in fields) +
            "".join('printf("%%d ", (int)%s);' % c for c in consts) + 'printf("%.17g %.17g\\n", VPGO_SMALL_ANGLE, VPGO_LAMBDA_FLOOR);return 0;}\n')
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "s.c"), "w").write(prog)
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), os.path.join(d, "s.c"), "-o", os.path.join(d, "s")])
        out = subprocess.check_output([os.path.join(d, "s")]).decode().split()
    pg = posegraph
    mirror = {"vpgo_options": pg.VpgoOptions, "vpgo_summary": pg.VpgoSummary}
    assert [C.sizeof(mirror[s]) for s in structs] + [getattr(mirror[s], f).offset for s, f in fields] + [
        len(pg.KERNELS), pg.SEGMENT, pg.MAX_SEPARATORS, pg.SUM_BLOCK, pg.MAX_ITERATIONS, pg.PRIOR, pg.BETWEEN, pg.POSITION, pg.TERM_NONE, pg.TERM_STEP, pg.TERM_COST,
        pg.TERM_MAX_ITERATIONS, pg.ERR_CAPACITY] == [int(v) for v in out[:-2]]
    assert [float(v) for v in out[-2:]] == [pg.SMALL_ANGLE, pg.LAMBDA_FLOOR]
    # the restatement states the same constants on its own
    assert (posegraph_ref.SEGMENT, posegraph_ref.SUM_BLOCK, posegraph_ref.SMALL_ANGLE, posegraph_ref.LAMBDA_FLOOR) == (pg.SEGMENT, pg.SUM_BLOCK, pg.SMALL_ANGLE, pg.LAMBDA_FLOOR)
    o = pg.default_options(lib.load_vilsolve())
    assert (o.max_iterations, o.initial_lambda, o.step_tolerance, o.cost_tolerance) == (20, 1e-5, 1e-10, 1e-12)


def test_create_checks_its_arguments_first_and_refuses_without_device():
    """No device (or, on a GPU machine, a device index that does not exist): VIL_ERR_DEVICE, there is no CPU fallback.  A size that is
    not positive is VIL_ERR_INVALID_ARGUMENT with or without a device."""
    import torch
    so = lib.load_vilsolve()
    nodev = 1 << 20 if torch.cuda.is_available() else 0
    with pytest.raises(posegraph.PoseGraphError) as e:
        posegraph.PoseGraph(so, max_poses=16, max_factors=16, device=nodev)
    assert e.value.status == -2
    for n, f in ((0, 16), (-5, 16), (16, 0), (16, -1)):
        with pytest.raises(posegraph.PoseGraphError) as e:
            posegraph.PoseGraph(so, max_poses=n, max_factors=f, device=nodev)
        assert e.value.status == -1, (n, f)
    fn = so.vpgo_create; fn.restype = C.c_int
    assert fn(C.c_int32(nodev), C.c_int32(16), C.c_int32(16), None) == -1


@pytest.mark.skipif(not (os.path.exists(os.path.join(LLVM, "llvm-objdump")) and os.path.exists(os.path.join(LLVM, "llvm-readelf"))), reason="needs the ROCm LLVM tools")
def test_posegraph_kernels_do_not_spill_vector_registers():
    """Read from the code object's notes, as test_loopverify_abi.py does: no spill, no scratch, <= 128 vector registers, <= 160 kB of LDS."""
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
    assert len(posegraph.KERNELS) == 11
    for k in posegraph.KERNELS:
        hit = [n for n in seen if re.search(r"\d%sE" % k, n)]           # the mangled name: length, name, E
        assert len(hit) == 1, (k, sorted(seen))
        spill, scratch, vgprs, lds = seen[hit[0]]
        print(k, "vgprs", vgprs, "lds", lds)
        assert spill == 0 and scratch == 0, "%s spills %d vector registers (%d B of scratch per lane)" % (k, spill, scratch)
        assert vgprs <= 128 and lds <= 160 * 1024, (k, vgprs, lds)
