"""No-GPU checks of include/vilgmap.h (the resident global map): libvilsolve.so exports every declared symbol, the ctypes mirrors have the
C compiler's layout, vgmap_create checks its arguments and then refuses to run without a device, and none of the row's kernels spills
vector registers."""
import ctypes as C
import os
import re
import shutil
import subprocess
import tempfile

import pytest

from mvil_fusion_amd import globalmap, lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LLVM = "/opt/rocm/lib/llvm/bin"


def test_library_exports_every_vgmap_symbol():
    so = lib.load_vilsolve()
    src = open(os.path.join(ROOT, "include", "vilgmap.h")).read()
    syms = sorted(set(re.findall(r"\b(vgmap_[a-z_0-9]+)\s*\(", src)))
    assert syms == ["vgmap_add_scan", "vgmap_clear", "vgmap_create", "vgmap_default_config", "vgmap_default_ref_options", "vgmap_destroy", "vgmap_get_points", "vgmap_insert",
                    "vgmap_insert_key", "vgmap_profile_enable", "vgmap_profile_read", "vgmap_rebuild", "vgmap_reference", "vgmap_size"], syms
    for s in syms:
        assert hasattr(so, s), "libvilsolve.so does not export %s" % s


def test_struct_layout_constants_and_defaults_match_header():
    fields = [("vgmap_config", "max_ref_points"), ("vgmap_config", "map_resolution"), ("vgmap_config", "origin"), ("vgmap_ref_options", "k"), ("vgmap_ref_options", "radius"),
              ("vgmap_ref_options", "ref_resolution"), ("vgmap_ref_options", "max_dist")]
    structs = ["vgmap_config", "vgmap_ref_options"]
    prog = ('#include <stdio.h>\n#include <stddef.h>\n#include "vilgmap.h"\nint main(void){' +
            "".join('printf("%%zu ", sizeof(%s));' % s for s in structs) + "".join('printf("%%zu ", offsetof(%s, %s));' % f for f in fields) +
            'printf("%d %d %d %d %d\\n", VGMAP_NUM_KERNELS, VGMAP_MAX_K, VGMAP_VOXEL_LIMIT, VGMAP_REF_RADIUS, VGMAP_REF_KNN);return 0;}\n')
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "s.c"), "w").write(prog)
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), os.path.join(d, "s.c"), "-o", os.path.join(d, "s")])
        out = [int(v) for v in subprocess.check_output([os.path.join(d, "s")]).decode().split()]
    gm = globalmap
    mirror = {"vgmap_config": gm.VgmapConfig, "vgmap_ref_options": gm.VgmapRefOptions}
    assert [C.sizeof(mirror[s]) for s in structs] + [getattr(mirror[s], f).offset for s, f in fields] + [len(gm.KERNELS), gm.MAX_K, gm.VOXEL_LIMIT, gm.REF_RADIUS, gm.REF_KNN] == out
    so = lib.load_vilsolve()
    g = gm.default_config(so)
    assert (g.max_map_points, g.max_scan_points, g.max_keys, g.max_keyed_points, g.max_ref_points) == (1 << 22, 1 << 17, 4096, 1 << 24, 1 << 18)
    assert g.map_resolution == C.c_float(0.05).value and list(g.origin) == [0.0, 0.0, 0.0]           # util.h:79
    o = gm.default_ref_options(so)
    assert (o.mode, o.k, o.radius, o.ref_resolution, o.max_dist) == (gm.REF_RADIUS, 5, 0.5, C.c_float(0.3).value, 1.5)        # util.h:80, :81; globalMappingIkdTree.cpp:686
    assert gm.default_ref_options(so, mode="knn", k=3).mode == gm.REF_KNN
    with pytest.raises(AttributeError):
        gm.default_config(so, no_such_field=1)


def test_create_checks_its_arguments_first_and_refuses_without_device():
    """No device (or, on a GPU machine, a device index that does not exist): VIL_ERR_DEVICE, there is no CPU fallback.  A bad
    configuration is VIL_ERR_INVALID_ARGUMENT with or without a device."""
    import torch
    so = lib.load_vilsolve()
    nodev = 1 << 20 if torch.cuda.is_available() else 0
    small = dict(max_map_points=1024, max_scan_points=256, max_keys=4, max_keyed_points=1024, max_ref_points=256)
    with pytest.raises(globalmap.GlobalMapError) as e:
        globalmap.GlobalMap(so, device=nodev, **small)
    assert e.value.status == -2
    for bad in (dict(max_map_points=0), dict(max_scan_points=-1), dict(max_keys=0), dict(max_keyed_points=0), dict(max_ref_points=0), dict(map_resolution=float("nan")),
                dict(origin=(0.0, float("inf"), 0.0)), dict(max_map_points=(1 << 29) + 1)):
        with pytest.raises(globalmap.GlobalMapError) as e:
            globalmap.GlobalMap(so, device=nodev, **dict(small, **bad))
        assert e.value.status == -1, bad
    f = so.vgmap_create; f.restype = C.c_int
    cfg = globalmap.default_config(so, **small)
    assert f(C.c_int32(nodev), C.byref(cfg), None) == -1
    assert f(C.c_int32(nodev), None, C.byref(C.c_void_p())) == -1


@pytest.mark.skipif(not (os.path.exists(os.path.join(LLVM, "llvm-objdump")) and os.path.exists(os.path.join(LLVM, "llvm-readelf"))), reason="needs the ROCm LLVM tools")
def test_globalmap_kernels_do_not_spill_vector_registers():
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
    assert len(globalmap.DEVICE_KERNELS) == 12
    for k in globalmap.DEVICE_KERNELS:
        hit = [n for n in seen if k in n]
        assert len(hit) == 1, (k, sorted(seen))
        spill, scratch, vgprs, lds = seen[hit[0]]
        print(k, "vgprs", vgprs, "lds", lds)
        assert spill == 0 and scratch == 0, "%s spills %d vector registers (%d B of scratch per lane)" % (k, spill, scratch)
        assert vgprs <= 128 and lds <= 160 * 1024, (k, vgprs, lds)
