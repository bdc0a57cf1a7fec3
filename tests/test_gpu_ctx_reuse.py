"""One solver context through its growth paths: every device resource of vil_ctx is grow-only and owned by the context, so a context that has
grown (arena, pinned image, mirror, chain table, marginalisation work space, pinned scratch, IMU permutation, LiDAR slab tables) and is then
reused while oversized computes, bit for bit, what a freshly created context computes; and creating and destroying contexts loses no memory per cycle."""
import copy

import numpy as np
import pytest
import torch

from mvil_fusion_amd import abi, lib, replay, synth
from mvil_fusion_amd.abi import Window

pytestmark = pytest.mark.gpu

# no host-timed cap: the iteration count must not depend on the wall clock
OPTS = dict(max_iterations=8, max_time_s=0.0)
CLASSES = (abi.FACTOR_IMU, abi.FACTOR_VISUAL, abi.FACTOR_EDGE, abi.FACTOR_PLANE)


def _small(base):
    """The K = 2 window of test_gpu_edge.test_minimal_window_two_frames."""
    w = Window(2, 12)
    w.pose, w.speedbias = base.pose[:2].copy(), base.speedbias[:2].copy()
    w.ex_pose, w.td = base.ex_pose.copy(), base.td.copy()
    w.G, w.sqrt_info_px = base.G.copy(), base.sqrt_info_px
    w.imu_i, w.imu_j, w.imu_const = np.array([0], np.int32), np.array([1], np.int32), base.imu_const[:1].copy()
    sel = np.where((base.vis_i == 0) & (base.vis_j == 1))[0][:12]
    w.vis_i, w.vis_j, w.vis_l = base.vis_i[sel].copy(), base.vis_j[sel].copy(), np.arange(len(sel), dtype=np.int32)
    w.vis_const = base.vis_const[sel].copy()
    w.L = len(sel); w.inv_depth = base.inv_depth[base.vis_l[sel]].copy(); w.lm_const = np.zeros(w.L, np.uint8)
    return w


def _solve(be, w0):
    w = copy.deepcopy(w0)
    sm = be.solve(w, abi.default_options(**OPTS))
    return [w.pose, w.speedbias, w.ex_pose, w.td, w.inv_depth, np.array([sm.initial_cost, sm.final_cost]), np.array([sm.iterations, sm.termination])]


def _marginalize(be, w0):
    out = be.marginalize(copy.deepcopy(w0), abi.MARGIN_OLD, opts=abi.default_options(**OPTS))
    return [np.array([out.c.n, out.c.nblk, out.c.m]), out.blk_kind, out.blk_index, out.blk_col, out.x0, out.J0, out.r0, out.A, out.b]


def _eval(cls):
    return lambda be, w0: list(be.eval_factors(copy.deepcopy(w0), cls, jac=True))


def _same(name, got, want):
    assert len(got) == len(want)
    for q, (a, b) in enumerate(zip(got, want)):
        a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
        assert a.shape == b.shape and a.tobytes() == b.tobytes(), (name, q)


def test_grown_context_reused_equals_fresh_context():
    """small -> large (solve, marginalize, eval_factors with Jacobians) -> small on ONE context; every call against the same call on a fresh context."""
    big = synth.make_config(1, n_plane=2000, n_edge=600)       # config 1's window with LiDAR points: every factor table of the arena is present
    small = _small(synth.make_config(1))
    assert small.L >= 3 and len(big.plane_pose) == 2000 and len(big.edge_pose) == 600
    calls = [("small", _solve, small), ("large", _solve, big), ("large marginalize", _marginalize, big)]
    calls += [("large eval %d" % c, _eval(c), big) for c in CLASSES]
    calls += [("small again", _solve, small)]
    fresh = []
    for name, fn, w in calls:
        be = lib.open_vilsolve()
        fresh.append(fn(be, w))
        be.close()
    be = lib.open_vilsolve()
    for (name, fn, w), want in zip(calls, fresh):
        _same(name, fn(be, w), want)
    be.close()
    assert fresh[2][0][0] > 0                                 # a prior came out of the marginalisation
    assert all(len(f[0]) > 0 and len(f[1]) > 0 for f in fresh[3:3 + len(CLASSES)])


def test_slab_growth_with_live_slabs_equals_fresh_context():
    """Three frames of 200 plane / 100 edge points, then one of 3000 / 1500: the slab tables grow while three slabs are live and are copied."""
    K = 4
    rp = replay.Replay(K=K, n_frames=K + 4, L=60, n_plane=K * 3000, n_edge=K * 1500, seed=5, max_iterations=8)
    rp.opts.max_time_s = 0.0
    frames = [(rp.lidar[k][0][:200], rp.lidar[k][1][:100]) for k in range(K - 1)] + [(rp.lidar[K - 1][0][:3000], rp.lidar[K - 1][1][:1500])]
    assert [(len(p), len(e)) for p, e in frames] == [(200, 100)] * 3 + [(3000, 1500)]
    w0 = rp.window(with_lidar=False)

    def run():
        be = lib.open_vilsolve()
        be.lidar_reset()
        for p, e in frames:
            be.lidar_push(p, e)
        w = copy.deepcopy(w0)
        sm = be.solve(w, rp.opts)
        be.close()
        return [w.pose, w.speedbias, w.ex_pose, w.td, w.inv_depth, np.array([sm.iterations, sm.termination])]

    a = run()
    _same("resident solve", run(), a)
    assert a[5][0] > 0 and np.abs(a[0] - w0.pose).max() > 0    # the solve moved the state


def test_create_destroy_churn_loses_no_memory_per_cycle():
    w0 = synth.make_config(1)
    free = [torch.cuda.mem_get_info()[0]]
    for half in range(2):
        for _ in range(8):
            be = lib.open_vilsolve()
            be.solve(copy.deepcopy(w0), abi.default_options(**OPTS))
            be.close()
        free.append(torch.cuda.mem_get_info()[0])
    first, second = free[0] - free[1], free[1] - free[2]
    print("create / solve / destroy: free device memory lost in cycles 1-8: %d bytes, in cycles 9-16: %d bytes" % (first, second))
    assert second <= first
