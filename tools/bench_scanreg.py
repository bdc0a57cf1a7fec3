"""Per-scan wall time and per-kernel HIP-event time of vscan_extract (include/vilscan.h) on the 16-ring x 1800 and 64-ring x 1800
synthetic scans, written to profiles/scanreg.txt (OUT=<file> for another place) with the box and the commit.

    python tools/bench_scanreg.py [calls, default 300]

Wall time is taken with the profiling events off, kernel times in a second pass with them on.  There is no compiled CPU counterpart of
this stage: the only CPU restatement is the Python one of tests/scanreg_ref.py, which is test infrastructure and not a timing baseline."""
import os
import socket
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import __graft_entry__ as g; g.load_package()
from mvil_fusion_amd import lib, scanreg
from mvil_fusion_amd.vgicp import _rot
from _rowbench import WARM, commit, device_name, profiled, timed, write

N = max(200, int(sys.argv[1])) if len(sys.argv) > 1 else 300
OUT = os.environ.get("OUT") or os.path.join(ROOT, "profiles", "scanreg.txt")


so = lib.load_vilsolve()
lines = ["vscan_extract, %d warm calls per figure after %d warm-up calls; box %s (%s); commit %s" % (N, WARM, socket.gethostname(), device_name(), commit()),
         "wall = host clock around the call (upload, four kernels, read-back, copy-out), events off; kernel = HIP events, second pass",
         "no CPU timing baseline exists for this stage: the only CPU restatement is tests/scanreg_ref.py (Python, test infrastructure)"]
R, t = _rot(-0.01, 0.015, -0.7), np.array([-2.0, 1.5, 0.2])
for rings, lo, hi in ((16, -15.0, 15.0), (64, -24.9, 2.0)):
    raw = scanreg.make_raw_scan(R, t, seed=1, rings=rings, az=1800, lower=lo, upper=hi)
    reg = scanreg.ScanReg(so, scanreg.default_config(so, num_rings=rings, lower_bound_deg=lo, upper_bound_deg=hi), max_points=len(raw))
    f, wall = timed(lambda: reg.extract(raw), N)
    kernels = profiled(reg, lambda: reg.extract(raw), N, unit="scan")
    reg.close()
    lines.append("%d rings x 1800 (%d points; %d sharp, %d less sharp, %d flat, %d less flat of %d before the filter): %s" %
                 (rings, len(raw), len(f.corner_sharp), len(f.corner_less_sharp), len(f.surf_flat), len(f.surf_less_flat), f.n_less_flat_raw, wall))
    lines += kernels
write(lines, OUT)
