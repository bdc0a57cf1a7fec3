"""Per-call wall time and per-kernel HIP-event time of vdepth_register (include/vildepth.h) against a resident cloud: about 100 k points
with 150 features (what the tracker node holds: 5 s of scans, one image) and about 400 k points with 600 features, written to
profiles/depthreg.txt (OUT=<file> for another place) with the device and the commit.

    python tools/bench_depthreg.py [calls, default 300]

Wall time is taken with the profiling events off, kernel times in a second pass with them on.  The cloud is uploaded once, outside the
timed calls, as the node does it (once per LiDAR scan, not per image); vdepth_set_cloud is timed on its own.  There is no compiled CPU
counterpart of this stage (PCL is absent): the only CPU restatement is the Python one of tests/depthreg_ref.py, which is test
infrastructure and not a timing baseline, so no speed-up is claimed."""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import __graft_entry__ as g; g.load_package()
from mvil_fusion_amd import depthreg, lib
from mvil_fusion_amd.vgicp import _rot
from _rowbench import WARM, commit, device_name, profiled, timed, write

N = max(200, int(sys.argv[1])) if len(sys.argv) > 1 else 300
OUT = os.environ.get("OUT") or os.path.join(ROOT, "profiles", "depthreg.txt")


so = lib.load_vilsolve()
lines = ["vdepth_register, %d warm calls per figure after %d warm-up calls; %s; commit %s" % (N, WARM, device_name(), commit()),
         "wall = host clock around the call (upload of matrices + features, two clears, three kernels, read-back), events off; kernel = HIP events, second pass",
         "no CPU timing baseline exists for this stage: the only CPU restatement is tests/depthreg_ref.py (Python, test infrastructure)"]
R, t = _rot(0.02, -0.03, 0.4), np.array([1.0, -2.0, 0.2])
for n_poses, az, n_feat in ((7, 900, 150), (14, 1800, 600)):
    cloud, feat, _ = depthreg.make_scene(R, t, seed=1, n_poses=n_poses, az=az, n_feat=n_feat)
    m1, m2 = depthreg.view_matrices(R, t, *depthreg.EXTRINSIC)
    reg = depthreg.DepthReg(so, max_cloud_points=len(cloud), max_features=n_feat)
    up = []
    for _ in range(WARM):
        a = time.perf_counter(); reg.set_cloud(cloud); up.append(time.perf_counter() - a)
    d, wall = timed(lambda: reg.register(m1, m2, feat), N)
    kernels = profiled(reg, lambda: reg.register(m1, m2, feat), N)
    reg.close()
    lines.append("%d points, %d features (%d in view, %d sphere points, %d with depth): %s; vdepth_set_cloud median %.3f ms" %
                 (len(cloud), n_feat, d.n_in_view, d.n_sphere, d.n_with_depth, wall, 1e3 * np.median(up[5:])))
    lines += kernels
write(lines, OUT)
