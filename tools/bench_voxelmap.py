"""Per-call wall time of feeding vgicp_align a new target (include/vilvgicp.h, include/vilvgicp_voxel.h) under the host builder and the device
builder of the voxel map, on the synthetic scan pair at 2.4 k, 14.4 k and 57.6 k points: vgicp_set_target with the covariances given and
with NULL, vgicp_covariances alone (the covariance share of a NULL call), vgicp_promote_source, the device builder's per-kernel HIP-event
times, vloop_verify over 1 and 8 candidates under both builders, and the degenerate cloud of 14.4 k points in ONE voxel.  Written to
profiles/voxelmap.txt (OUT=<file> for another place) with the device and the commit.

    python tools/bench_voxelmap.py [calls, default 100]

Every step runs in a child process of its own under a time limit of its own; a step that fails or runs out of time ends the run, what
was measured until then is still written.  Wall time is taken with the profiling events off, kernel times in a second pass with them on.
The host builder IS the parent commit's path, unchanged: it is the baseline, measured in the same process as the device builder."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import __graft_entry__ as g; g.load_package()
from mvil_fusion_amd import lib, loopverify as lv, vgicp
from _rowbench import WARM, commit, device_name, profiled, timed, write

OUT = os.environ.get("OUT") or os.path.join(ROOT, "profiles", "voxelmap.txt")
STEPS = (("build", 150, 240), ("build", 900, 300), ("build", 3600, 420), ("verify", 150, 300), ("onevoxel", 900, 300))     # (what, azimuths of 16 rings, time limit in s)
KERNEL_FMT = "    %-14s %5d launches, %9.2f us per launch"
BUILDERS = (("host builder", vgicp.BUILD_HOST), ("device builder", vgicp.BUILD_DEVICE))


class BuildProfile:
    """The builder's profiler behind the names _rowbench.profiled() calls."""

    def __init__(self, reg):
        self.profile_enable, self.profile_read = reg.build_profile_enable, reg.build_profile_read


def step_build(az, calls):
    tx, tc, sx, sc, _ = vgicp.make_pair(0, rings=16, az=az)
    n = len(tx)
    k = calls if n < 20000 else max(20, calls // 2)
    reg = vgicp.Vgicp(lib.load_vilsolve())
    lines = []
    for name, builder in BUILDERS:
        reg.set_voxel_builder(builder)
        for what, cov in (("covariances given", tc), ("covariances NULL", None)):
            _, wall = timed(lambda: reg.set_target(tx, cov), k)
            lines.append("vgicp_set_target, %d points, %s, %s (%d voxels), %d calls: %s" % (n, name, what, len(reg.read_voxels()["keys"]), k, wall))
    _, wall = timed(lambda: reg.covariances(tx), k)
    lines.append("vgicp_covariances alone, %d points (upload, estimate, 72 B per point down), %d calls: %s" % (n, k, wall))
    reg.set_source(tx)
    _, wall = timed(lambda: reg.promote_source(0.5), k)
    lines.append("vgicp_promote_source, %d resident points (%d voxels), %d calls: %s" % (n, len(reg.read_voxels()["keys"]), k, wall))
    reg.set_voxel_builder(vgicp.BUILD_DEVICE)
    lines.append("device builder's kernels, %d points, covariances given, %d calls:" % (n, k))
    lines += profiled(BuildProfile(reg), lambda: reg.set_target(tx, tc), k, unit="build", fmt=KERNEL_FMT)
    reg.build_profile_enable(False)
    reg.close()
    return lines


def step_verify(az, calls):
    so = lib.load_vilsolve()
    tx, _, sx, _, _ = vgicp.make_pair(0, rings=16, az=az)
    ctx = lv.LoopVerify(so, max_points=len(sx)); reg = vgicp.Vgicp(so)
    opts = lv.default_options(so)
    lines = []
    for name, builder in BUILDERS:
        reg.set_voxel_builder(builder)
        for n_cand in (1, 8):
            cands = [(tx, np.eye(4))] * n_cand
            k = max(10, calls // (2 * n_cand))
            (best, per), wall = timed(lambda: ctx.verify(reg, sx, cands, opts), k)
            lines.append("vloop_verify, %s, query %d points, %d candidate(s) of %d points (winner %d, fitness %.6g, %d iterations), %d calls: %s" %
                         (name, len(sx), n_cand, len(tx), best.index, best.fitness, per[0].iterations, k, wall))
    ctx.close(); reg.close()
    return lines


def step_onevoxel(az, calls):
    n = 16 * az
    rng = np.random.default_rng(0)
    xyz = (np.array([1.5, 2.5, 0.5]) * 0.5 + rng.uniform(0.0, 0.2, (n, 3))).astype(np.float32)
    cov = rng.uniform(-1.0, 1.0, (n, 9))
    reg = vgicp.Vgicp(lib.load_vilsolve())
    k = max(20, calls // 2)
    lines = []
    for name, builder in BUILDERS:
        reg.set_voxel_builder(builder)
        _, wall = timed(lambda: reg.set_target(xyz, cov), k)
        lines.append("vgicp_set_target, %d points in ONE voxel (%d voxels), %s, covariances given, %d calls: %s" % (n, len(reg.read_voxels()["keys"]), name, k, wall))
    lines.append("device builder's kernels, %d points in ONE voxel (one serial run of %d additions per component), %d calls:" % (n, n, k))
    lines += profiled(BuildProfile(reg), lambda: reg.set_target(xyz, cov), k, unit="build", fmt=KERNEL_FMT)
    reg.build_profile_enable(False)
    reg.close()
    return lines


if __name__ == "__main__":
    if len(sys.argv) > 4 and sys.argv[1] == "--step":
        fn = {"build": step_build, "verify": step_verify, "onevoxel": step_onevoxel}[sys.argv[2]]
        print("\n".join(fn(int(sys.argv[3]), int(sys.argv[4]))))
        sys.exit(0)
    calls = max(20, int(sys.argv[1])) if len(sys.argv) > 1 else 100
    lines = ["target voxel map of the VGICP row (include/vilvgicp.h, include/vilvgicp_voxel.h), each figure over the calls its line names, after %d warm-up calls; %s; commit %s" %
             (WARM, device_name(), commit()),
             "wall = host clock around the call (every call ends in a host wait), events off; kernel = HIP events, second pass",
             "the host builder is the path of the parent commit, unchanged, measured in the same process; resolution 0.5 m; 16 rings x 150 / 900 / 3600 azimuths"]
    for what, az, limit in STEPS:
        try:
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--step", what, str(az), str(calls)], capture_output=True, text=True, timeout=limit)
        except subprocess.TimeoutExpired:
            lines.append("%s %d: no result within %d s; the run ends here" % (what, 16 * az, limit))
            break
        if p.returncode != 0:
            lines.append("%s %d: exit status %d; the run ends here\n%s" % (what, 16 * az, p.returncode, p.stderr[-1000:]))
            break
        lines.append(p.stdout.rstrip("\n"))
    write(lines, OUT)
