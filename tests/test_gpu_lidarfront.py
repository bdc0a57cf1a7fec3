"""GPU checks of include/vilfront.h (processLidar as one resident call), through the C-ABI.

The de-skew is transcendental (acosf, sinf): its coordinates are compared with 50-digit values (tests/lidarfront_ref.py) under the
project's "16 x the floor" rule, the floor being the float32 NumPy restatement's own worst error on the same fixture; the kept mask, the
order, the counts and the intensities are compared exactly.  Everything after the de-skew is compared on raw bytes with the chain of the
library's public calls fed the device's own de-skewed cloud."""
import hashlib
import os
import subprocess
import sys

import numpy as np
import pytest

import lidarfront_ref as R
from mvil_fusion_amd import cloud, lib, lidarfront, loopverify, vgicp

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = (1, 63, 64, 65, 256, 257, 1025)       # wave edges, one workgroup +- 1, more than four workgroups + 1
MAXPTS = 4096
GRID_PAIR = 3                                 # the pair of the chain that is scored through the search grid (min_points lowered to 512)
FLOOR_FACTOR = 16.0


def raw_bytes(a):
    return np.ascontiguousarray(a).view(np.uint8)


def same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(raw_bytes(a), raw_bytes(b))


@pytest.fixture(scope="module")
def so():
    return lib.load_vilsolve()


@pytest.fixture(scope="module")
def front(so):
    f = lidarfront.LidarFront(so, max_scan_points=MAXPTS)
    yield f
    f.close()


def push(f, k, **kw):
    """Scan k of the chain into f; the grid pair with the lowered threshold on."""
    xyzi, q, t, g = R.chain()[k]
    f.set_grid(512 if k == GRID_PAIR else 1024, 0.5)
    return f.push_scan(xyzi, lidarfront.motion(q, t), kw.pop("guess", g if k else None), kw.pop("opts", None))


def chain_digest(f, n=6):
    f.reset()
    h = hashlib.sha256()
    for k in range(n):
        s = push(f, k)
        h.update(lidarfront.summary_bytes(s)); h.update(f.read_deskewed().tobytes()); h.update(f.debug_read(lidarfront.DBG_FILTERED).tobytes())
    return h.hexdigest()


# ---- de-skew and compaction ----------------------------------------------------------------------------------------------------------
def _check_deskew(f, xyzi, q, t, exact, out_ref, keep, floor, label):
    """One push of xyzi on a reset context; returns the worst |device - 50 digits| / floor."""
    f.reset()
    s = f.push_scan(xyzi, lidarfront.motion(q, t))
    dev = f.read_deskewed()
    assert (s.n_raw, s.n_kept, s.aligned) == (len(xyzi), int(keep.sum()), 0), label
    assert dev.shape == (int(keep.sum()), 4) and dev.dtype == np.float32
    assert same(dev[:, 3], out_ref[keep][:, 3]), label                                              # the truncated intensities, in order
    assert same(dev, f.debug_read(lidarfront.DBG_DESKEWED))
    if not keep.any():
        return 0.0
    err = R.abs_err(dev[:, :3], exact[keep])                                                        # every kept point, every coordinate
    ratio = float(err.max() / floor)
    print(label, "kept", int(keep.sum()), "of", len(xyzi), "worst |device - exact|", err.max(), "floor", floor, "ratio", ratio)
    bad = np.argwhere(err > FLOOR_FACTOR * floor)
    assert len(bad) == 0, (label, "kept points (index, coordinate) beyond 16 x the floor, which is also what a wrong mask or order gives", bad[:8].tolist(), ratio)
    return ratio


@pytest.mark.parametrize("n", SIZES)
def test_deskew_prefixes_match_the_restatement(front, n):
    xyzi, q, t, exact, out_ref, keep = R.prefix_scan()
    floor = R.abs_err(out_ref[keep][:, :3], exact[keep]).max()                                      # of the float32 restatement, on the whole fixture
    _check_deskew(front, xyzi[:n], q, t, exact[:n], out_ref[:n], keep[:n], floor, "prefix n=%d" % n)


def test_deskew_branch_fixture_matches_the_restatement(front):
    cases = []
    for name, xyzi, q, t in R.branch_fixture():
        out_ref, keep, info = R.deskew_f32(xyzi, q, t)
        cases.append((name, xyzi, q, t, R.deskew_mp(xyzi, q, t, keep=keep), out_ref, keep))
    floor = max(R.abs_err(c[5][c[6]][:, :3], c[4][c[6]]).max() for c in cases)                      # one fixture: the floor is over its three motions
    for name, xyzi, q, t, exact, out_ref, keep in cases:
        _check_deskew(front, xyzi, q, t, exact, out_ref, keep, floor, "branches/" + name)


def test_all_rejected_scan_is_not_accepted_and_leaves_the_pair_alone(so, front):
    xyzi, q, t, _ = R.chain()[1]
    bad = xyzi.copy(); bad[:, 3] = -bad[:, 3] - 0.5                                                 # every s < 0
    twin = lidarfront.LidarFront(so, max_scan_points=MAXPTS)
    front.reset()
    a0, b0 = push(front, 0), push(twin, 0)
    s = front.push_scan(bad, lidarfront.motion(q, t), R.chain()[1][3])
    assert (s.n_raw, s.n_kept, s.n_filtered, s.accepted, s.aligned) == (len(bad), 0, 0, 0, 0)
    assert len(front.read_deskewed()) == 0 and len(front.debug_read(lidarfront.DBG_FILTERED)) == 0
    s = front.push_scan(np.zeros((0, 4), np.float32), lidarfront.motion(q, t))                      # and an empty one
    assert (s.n_raw, s.n_kept, s.accepted) == (0, 0, 0)
    a1, b1 = push(front, 1), push(twin, 1)
    twin.close()
    assert lidarfront.summary_bytes(a0) == lidarfront.summary_bytes(b0) and lidarfront.summary_bytes(a1) == lidarfront.summary_bytes(b1)
    assert a1.aligned == 1 and a1.accepted == 1


def test_deskew_off_passes_the_raw_scan_through(so, front):
    raw = R.branch_points()                                                                         # NaNs and all
    front.reset()
    o = lidarfront.default_options(so, deskew=0)
    s = front.push_scan(raw, None, None, o)
    assert (s.n_raw, s.n_kept, s.accepted) == (len(raw), len(raw), 1)
    assert same(front.read_deskewed(), raw)
    dc = cloud.DepthCloud(so, max_scan_points=MAXPTS, max_scans=1)
    assert same(front.debug_read(lidarfront.DBG_FILTERED), dc.filter(raw, o.leaf, o.hist_size))      # filter A drops the non-finite points itself
    dc.close()


# ---- everything after the de-skew, on raw bytes ----------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def fused_and_chain(so, front):
    """Six scans through vfront_push_scan, and through the public calls fed the device's own de-skewed clouds.  CONDITION OF THE FIXTURE:
    every pair of the chain converges (checked on the CPU with the oracle's VGICP restatement by tests/test_lidarfront_ref.py, asserted on
    the device below): a pair that does not converge would still have to agree, but would not exercise the path a caller takes."""
    front.reset()
    dc = cloud.DepthCloud(so, max_scan_points=MAXPTS, max_scans=1)
    reg = vgicp.Vgicp(so)
    lv = loopverify.LoopVerify(so, max_points=MAXPTS)
    o = lidarfront.default_options(so)
    fused, chained = [], []
    prev = None
    for k in range(6):
        xyzi, q, t, g = R.chain()[k]
        s = push(front, k)
        desk = front.read_deskewed().copy()
        fused.append((s, desk, front.debug_read(lidarfront.DBG_FILTERED).copy()))
        filt = dc.filter(desk, o.leaf, o.hist_size)
        rec = dict(filtered=filt)
        xyz = np.ascontiguousarray(filt[:, :3])
        if prev is not None:
            reg.set_voxel_builder(vgicp.BUILD_DEVICE if k % 2 else vgicp.BUILD_HOST)                # either builder
            reg.set_target(prev, None, o.resolution)
            reg.set_source(xyz, None)
            T, sm = reg.align(g.astype(np.float32).astype(np.float64), o.reg)
            T = T.astype(np.float32).astype(np.float64)
            lv.set_grid(512 if k == GRID_PAIR else 1024, 0.5)
            lv.set_target(prev); lv.set_source(xyz)
            fit, used = lv.score(T)
            rec.update(T=T, summary=sm, fitness=float(fit), n_used=int(used))
        chained.append(rec)
        prev = xyz
    dc.close(); reg.close(); lv.close()
    return fused, chained


def test_chain_of_public_calls_gives_the_same_bytes(fused_and_chain):
    fused, chained = fused_and_chain
    for k, ((s, desk, filt), rec) in enumerate(zip(fused, chained)):
        assert s.accepted == 1 and s.aligned == (1 if k else 0) and s.n_filtered == len(filt) and s.n_kept == len(desk), k
        assert 0 < len(filt) < 1024, "the filtered clouds stay below vloop's default grid threshold"
        assert (len(filt) >= 512) if k == GRID_PAIR else True
        assert same(filt, rec["filtered"]), k
        if not k:
            assert same(loopverify.mat(s.T), np.eye(4)) and s.fitness == 0.0 and s.n_used == 0
            continue
        assert s.reg.converged == 1, "pair %d does not converge: the fixture's condition" % k
        assert same(loopverify.mat(s.T), rec["T"]), k
        assert np.float64(s.fitness).tobytes() == np.float64(rec["fitness"]).tobytes() and s.n_used == rec["n_used"], k
        assert lidarfront.summary_bytes(s.reg) == lidarfront.summary_bytes(rec["summary"]), k           # every field of the vgicp_summary
        assert s.n_used == len(filt) and 0.0 < s.fitness < 1.0


def test_null_guess_is_identity_and_a_guess_is_rounded_to_float(so, front):
    def second(guess):
        front.reset()
        push(front, 0)
        return lidarfront.summary_bytes(push(front, 1, guess=guess))
    assert second(None) == second(np.eye(4))
    g = R.chain()[1][3].copy()
    g[:3, :] += 1e-11 * np.arange(12).reshape(3, 4)                                                  # more than float precision
    g32 = g.astype(np.float32).astype(np.float64)
    assert not np.array_equal(g, g32) and second(g) == second(g32)


VILICP = r"""
#include <cstdio>
#include "vilicp_shim.hpp"
int main() {
    double in[1 + 16 + 16]; for (double& v : in) if (std::scanf("%la", &v) != 1) return 1;
    double ex[16]; for (int i = 0; i < 16; ++i) ex[i] = (i % 5 == 0) ? 1.0 : 0.0;
    ex[3] = 0.05; ex[7] = -0.02; ex[11] = 0.1;
    const vil::IcpConstraint c = vil::classify_icp_constraint(in[0], in + 1, in + 17, ex, true);
    std::printf("%d %d", c.mode, c.mode_applied);
    for (double v : c.lidar_trans) std::printf(" %a", v);
    for (double v : c.sqrt_info_diag) std::printf(" %a", v);
    std::printf("\n");
    return 0;
}
"""


def test_constraint_from_the_call_equals_constraint_from_the_chain(fused_and_chain, tmp_path):
    src = tmp_path / "c.cpp"; src.write_text(VILICP)
    exe = str(tmp_path / "c")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe])
    fused, chained = fused_and_chain

    def classify(fitness, guess, T):
        text = " ".join(float(v).hex() for v in [fitness] + list(np.asarray(guess).reshape(16)) + list(np.asarray(T).reshape(16)))
        return subprocess.run([exe], input=text, capture_output=True, text=True, check=True).stdout
    modes = set()
    for k in range(1, 6):
        g = R.chain()[k][3]
        a = classify(fused[k][0].fitness, g, loopverify.mat(fused[k][0].T))
        assert a == classify(chained[k]["fitness"], g, chained[k]["T"])
        modes.add(int(a.split()[0]))
    assert modes <= {2, 3} and modes, modes                                                          # a good fit of a moving sensor


# ---- errors leave the state alone ------------------------------------------------------------------------------------------------------
def test_refused_calls_leave_the_state_alone(so, front):
    twin = lidarfront.LidarFront(so, max_scan_points=MAXPTS)
    front.reset()
    a0, b0 = push(front, 0), push(twin, 0)
    desk, filt = front.read_deskewed().copy(), front.debug_read(lidarfront.DBG_FILTERED).copy()
    xyzi, q, t, g = R.chain()[1]
    m = lidarfront.motion(q, t)
    nanq = lidarfront.motion(q, t); nanq.q[2] = float("nan")
    nant = lidarfront.motion(q, t); nant.t[0] = float("inf")
    gbad = g.copy(); gbad[1, 3] = np.nan
    big = np.zeros((MAXPTS + 1, 4), np.float32)
    refused = [(big, m, g, None), (xyzi, nanq, g, None), (xyzi, nant, g, None), (xyzi, m, gbad, None), (xyzi, None, g, None)]
    for kw in (dict(hist_size=500), dict(hist_size=0), dict(hist_size=4096), dict(leaf=0.0), dict(leaf=-0.3), dict(leaf=float("nan")), dict(resolution=0.0),
               dict(lidar_time_step=0.0), dict(max_distance=float("inf")), dict(neighbor_mode=3), dict(rotation_epsilon=float("nan"))):
        refused.append((xyzi, m, g, lidarfront.default_options(so, **kw)))
    for args in refused:
        with pytest.raises(lidarfront.LidarFrontError) as e:
            front.push_scan(*args)
        assert e.value.status == lidarfront.ERR_INVALID_ARGUMENT
        assert same(front.read_deskewed(), desk) and same(front.debug_read(lidarfront.DBG_FILTERED), filt)
    a1, b1 = push(front, 1), push(twin, 1)
    twin.close()
    assert lidarfront.summary_bytes(a0) == lidarfront.summary_bytes(b0) and lidarfront.summary_bytes(a1) == lidarfront.summary_bytes(b1)
    assert a1.aligned == 1


# ---- reproducibility, profile -----------------------------------------------------------------------------------------------------------
CHILD = r"""
import sys
sys.path.insert(0, %r); sys.path.insert(0, %r)
import __graft_entry__ as graft
graft.load_package()
import test_gpu_lidarfront as T
from mvil_fusion_amd import lib, lidarfront
f = lidarfront.LidarFront(lib.load_vilsolve(), max_scan_points=T.MAXPTS)
print("digest", T.chain_digest(f))
f.close()
"""


def test_reproducible_across_contexts_and_processes(so, front):
    a = chain_digest(front)
    assert chain_digest(front) == a
    other = lidarfront.LidarFront(so, max_scan_points=5000)                                          # another context, another capacity
    assert chain_digest(other) == a
    other.close()
    code = CHILD % (ROOT, os.path.join(ROOT, "tests"))
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=120)      # a fresh child process, never an exec
    assert out.returncode == 0, out.stderr[-2000:]
    assert out.stdout.split()[-2:] == ["digest", a]


def test_profile_counts_every_kernel_once_per_call(front):
    front.reset()
    front.profile_enable(True)
    front.profile_read()
    for k in range(3):
        push(front, k)
    prof = front.profile_read()
    front.profile_enable(False)
    assert sorted(prof) == sorted(lidarfront.KERNELS)
    for k in lidarfront.KERNELS:
        assert prof[k][0] == 3 and prof[k][1] > 0.0, (k, prof)
    assert front.profile_read() == {k: (0, 0.0) for k in lidarfront.KERNELS}
