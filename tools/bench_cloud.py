"""Wall time, per-kernel HIP-event time and bytes moved of vcloud_push_scan (include/vilcloud.h) in the tracker node's steady state: a
16 x 1800 raw scan per push with 25 scans in the queue, written to profiles/cloud.txt (OUT=<file> for another place) with the device and
the commit.

    python tools/bench_cloud.py

Medians of 5 calls after the warm-up (the queue is filled and five more scans are pushed before anything is timed); wall time with the
profiling events off, kernel times from 5 more pushes with them on.  In the same run, on the same cloud: vdepth_set_cloud of the finished
depth cloud -- what the path without this row costs ON THE BUS ALONE, since there the host filters, queues and fuses and then uploads the
whole cloud -- and vcloud_publish.  The host's own filtering has no compiled implementation here (PCL is absent), so this is NOT a
speed-up claim against PCL.  Last: filter A at its worst case, every point in one voxel, where one thread adds the whole cloud."""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import __graft_entry__ as g; g.load_package()
from mvil_fusion_amd import cloud, depthreg, lib, scanreg
from mvil_fusion_amd.vgicp import _rot
from _rowbench import commit, device_name, write

OUT = os.environ.get("OUT") or os.path.join(ROOT, "profiles", "cloud.txt")
RINGS, AZ, LIVE, REPS = 16, 1800, 25, 5
DT = 0.205                                 # 5.0 / 0.205 = 24.4: a push finds 24 scans that stay, 25 are live after it
N_SCAN = RINGS * AZ


def scan_of(k):
    R = _rot(0.004 * (k % 40), -0.003 * (k % 40), 0.3 + 0.02 * k); t = np.array([-2.0 + 0.05 * (k % 60), 1.0 - 0.03 * (k % 60), 0.1])
    return np.ascontiguousarray(np.concatenate([R, t[:, None]], axis=1), np.float32), scanreg.make_raw_scan(R, t, seed=k, rings=RINGS, az=AZ)


def wall_of(fn, reps=REPS):
    ts = []
    for _ in range(reps):
        a = time.perf_counter(); fn(); ts.append(1e3 * (time.perf_counter() - a))
    return "wall median %8.3f ms, min %8.3f, max %8.3f" % (np.median(ts), min(ts), max(ts))


def kernel_lines(prof, calls):
    out = ["      %-16s %3d launches %9.3f ms per call" % (k, n, ms / calls) for k, (n, ms) in prof.items() if n]
    return out + ["      kernels together          %9.3f ms per call" % (sum(ms for _, ms in prof.values()) / calls)]


so = lib.load_vilsolve()
dc = cloud.DepthCloud(so, max_scan_points=N_SCAN, max_scans=LIVE + 1)
scans = [scan_of(k) for k in range(LIVE + 5 + 2 * REPS)]
k = 0
for _ in range(LIVE + 5):                                                                # warm-up: fill the queue, then steady state
    s = dc.push_scan(DT * k, *scans[k]); k += 1
assert s.n_scans == LIVE and s.n_popped == 1, cloud.counts(s)
walls = []
for _ in range(REPS):
    a = time.perf_counter(); s = dc.push_scan(DT * k, *scans[k]); walls.append(1e3 * (time.perf_counter() - a)); k += 1
dc.profile_enable(True); dc.profile_read()
for _ in range(REPS):
    s = dc.push_scan(DT * k, *scans[k]); k += 1
prof = dc.profile_read(); dc.profile_enable(False)
lines = ["vcloud_push_scan (include/vilcloud.h); %s; commit %s" % (device_name(), commit()),
         "%d x %d raw scan per push, %d scans live; medians of %d calls after %d warm-up pushes; wall = host clock around the call, events off; kernels = HIP events of %d more" %
         (RINGS, AZ, LIVE, REPS, LIVE + 5, REPS),
         "no compiled CPU opponent exists (PCL is no dependency of this project): this is no speed-up claim against PCL",
         "  last push: raw %d, down-sampled %d, in view %d, fused %d, depth cloud %d points" % (s.n_raw, s.n_scan_ds, s.n_in_view, s.n_fused, s.n_cloud),
         "  vcloud_push_scan                 wall median %8.3f ms, min %8.3f, max %8.3f" % (np.median(walls), min(walls), max(walls)),
         "      bytes up %d (the raw scan + 64 for the matrix), bytes back 64 (the header)" % (16 * s.n_raw + 64)]
lines += kernel_lines(prof, REPS)

world = dc.read_cloud()
reg = depthreg.DepthReg(so, max_cloud_points=len(world), max_features=16)
for _ in range(3):
    reg.set_cloud(world); dc.publish(reg)
lines.append("  vdepth_set_cloud, the same cloud   %s; bytes up %d: the bus share of the path that filters on the host" % (wall_of(lambda: reg.set_cloud(world)), 16 * len(world)))
lines.append("  vcloud_publish                   %s; device to device, nothing crosses the bus" % wall_of(lambda: dc.publish(reg)))
reg.close()

M, raw = scans[0]
dc.filter(raw, 0.2)
lines.append("  vcloud_filter, one raw scan      %s (%d -> %d points, leaf 0.2; includes the download of the result)" % (wall_of(lambda: dc.filter(raw, 0.2)), len(raw), len(dc.filter(raw, 0.2))))
rng = np.random.default_rng(0)
for n in (N_SCAN, s.n_fused, LIVE * N_SCAN):                                               # worst case: one voxel, one run, one thread's sum
    one = np.concatenate([rng.uniform(1.001, 1.199, (n, 3)), rng.uniform(0, 50, (n, 1))], axis=1).astype(np.float32)
    dc.filter(one, 0.2)
    dc.profile_enable(True); dc.profile_read()
    a = time.perf_counter(); m = len(dc.filter(one, 0.2)); w = 1e3 * (time.perf_counter() - a)
    p = dc.profile_read(); dc.profile_enable(False)
    lines.append("  vcloud_filter, %7d points in ONE voxel -> %d: wall %9.3f ms, k_cloud_emit %9.3f ms (one thread adds them all), the other kernels %7.3f ms" %
                 (n, m, w, p["k_cloud_emit"][1], sum(ms for kk, (_, ms) in p.items() if kk != "k_cloud_emit")))
dc.close()
write(lines, OUT)
