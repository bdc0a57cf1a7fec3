"""Wall time, per-kernel HIP-event time, bytes moved and host waits of vfront_push_scan (include/vilfront.h) against the chain of public
calls it composes, written to profiles/lidarfront.txt (OUT=<file> for another place) with the device and the commit.

    python tools/bench_lidarfront.py

A 16 x 1800 scan of a box room per call (tests/lidarfront_ref.py: room_scan), leaf 0.3 and leaf 0.5.  Per scan of one sequence, in the
same run and alternating: the fused call on one context; then, on three public contexts, vcloud_filter, vgicp_promote_source,
vgicp_set_source, vloop_set_target, vloop_set_source, vgicp_align and vloop_score, fed the NumPy de-skew of the same scan.  The chain
is reported with its NumPy de-skew excluded and included.  Medians after a warm-up; wall = host clock around calls that end in a device
synchronise, events off; the new kernels' times from HIP events in a second pass.  There is no compiled CPU opponent (no PCL, no fast_gicp
build): this is no speed-up claim against the reference."""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import __graft_entry__ as g; g.load_package()
import lidarfront_ref as R
from mvil_fusion_amd import cloud, lib, lidarfront, loopverify, vgicp
from _rowbench import commit, device_name, write

OUT = os.environ.get("OUT") or os.path.join(ROOT, "profiles", "lidarfront.txt")
RINGS, AZ, WARM, REPS = 16, 1800, 6, 15
N_SCAN = RINGS * AZ


def med(ts):
    ts = 1e3 * np.array(ts)
    return "median %8.3f ms, min %8.3f, max %8.3f" % (np.median(ts), ts.min(), ts.max())


so = lib.load_vilsolve()
scans = [R.room_scan(k, RINGS, AZ) for k in range(WARM + 2 * REPS)]
lines = ["vfront_push_scan (include/vilfront.h) against the chain of public calls; %s; commit %s" % (device_name(), commit()),
         "%d x %d scan per call; medians of %d scans after %d warm-up scans, the two paths alternating scan by scan; wall = host clock around the calls, events off" %
         (RINGS, AZ, REPS, WARM),
         "no compiled CPU opponent exists (neither PCL nor fast_gicp is a dependency of this project): this is no speed-up claim against the reference"]
for leaf in (0.3, 0.5):
    o = lidarfront.default_options(so, leaf=leaf)
    front = lidarfront.LidarFront(so, max_scan_points=N_SCAN)
    dc = cloud.DepthCloud(so, max_scan_points=N_SCAN, max_scans=1)
    reg = vgicp.Vgicp(so)
    lv = loopverify.LoopVerify(so, max_points=N_SCAN)
    t_fused, t_chain, t_numpy, prev, n_conv = [], [], [], None, 0
    for k in range(WARM + REPS):
        xyzi, q, t, guess = scans[k]
        mot = lidarfront.motion(q, t); gk = guess if k else None
        a = time.perf_counter(); s = front.push_scan(xyzi, mot, gk, o); b = time.perf_counter()
        out, keep, _ = R.deskew_f32(xyzi, q, t); desk = np.ascontiguousarray(out[keep]); c = time.perf_counter()
        filt = dc.filter(desk, leaf, o.hist_size)
        xyz = np.ascontiguousarray(filt[:, :3])
        if prev is not None:
            reg.promote_source(o.resolution)
        reg.set_source(xyz, None)
        if prev is not None:
            lv.set_target(prev)
        lv.set_source(xyz)
        if prev is not None:
            T, sm = reg.align(guess.astype(np.float32).astype(np.float64), o.reg)
            fit, used = lv.score(T.astype(np.float32).astype(np.float64))
        d = time.perf_counter()
        prev = xyz
        if k >= WARM:
            t_fused.append(b - a); t_numpy.append(c - b); t_chain.append(d - c)
            n_conv += int(s.aligned == 1 and s.reg.converged == 1 and sm.converged == 1)
    m, mp = len(filt), s.n_filtered
    front.profile_enable(True); front.profile_read()
    for k in range(WARM + REPS, WARM + 2 * REPS):
        xyzi, q, t, guess = scans[k]
        s = front.push_scan(xyzi, lidarfront.motion(q, t), guess, o)
    prof = front.profile_read(); front.profile_enable(False)
    grid = mp >= 1024
    lines += ["leaf %.1f: last scan raw %d, kept %d, filtered %d points (the chain's filter: %d); fitness %.6f over %d points, %d iterations; %d of %d timed pairs converged on both paths" %
              (leaf, s.n_raw, s.n_kept, s.n_filtered, m, s.fitness, s.n_used, s.reg.iterations, n_conv, REPS),
              "  vfront_push_scan                          wall %s" % med(t_fused),
              "      bytes up %d (the raw scan), bytes back 64 (the header) + the alignment's and the score's records; host waits %d" % (16 * s.n_raw, 8 if grid else 7),
              "  chain of public calls, de-skew excluded   wall %s" % med(t_chain),
              "  chain of public calls, NumPy de-skew in   wall %s" % med(np.array(t_chain) + np.array(t_numpy)),
              "      bytes up %d (the de-skewed cloud, the source twice, the fitness target), bytes back %d (the filtered cloud) + the same records; host waits %d and %d blocking copies" %
              (16 * s.n_kept + 12 * m * 3, 16 * m, 9 if grid else 8, 1),
              "      the NumPy de-skew alone               wall %s" % med(t_numpy)]
    lines += ["      %-16s %3d launches %9.3f ms per call" % (kk, n, ms / REPS) for kk, (n, ms) in prof.items()]
    lines += ["      new kernels together      %9.3f ms per call" % (sum(ms for _, ms in prof.values()) / REPS)]
    front.close(); dc.close(); reg.close(); lv.close()
write(lines, OUT)
