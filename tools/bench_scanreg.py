"""Per-scan wall time and per-kernel HIP-event time of vscan_extract (include/vilscan.h) on the 16-ring x 1800 and 64-ring x 1800
synthetic scans, written to profiles/scanreg.txt (OUT=<file> for another place) with the box and the commit.

    python tools/bench_scanreg.py [calls, default 300]

Wall time is taken with the profiling events off, kernel times in a second pass with them on.  There is no compiled CPU counterpart of
this stage: the only CPU restatement is the Python one of tests/scanreg_ref.py, which is test infrastructure and not a timing baseline."""
import os
import socket
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import __graft_entry__ as g; g.load_package()
from mvil_fusion_amd import lib, scanreg
from mvil_fusion_amd.vgicp import _rot

N = max(200, int(sys.argv[1])) if len(sys.argv) > 1 else 300
WARM = 20
OUT = os.environ.get("OUT") or os.path.join(ROOT, "profiles", "scanreg.txt")


def commit():
    try:
        return subprocess.check_output(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], stderr=subprocess.DEVNULL).decode().strip()
    except Exception:
        return os.environ.get("VIL_COMMIT", "unknown (not a git checkout)")


def device_name():
    import torch
    return torch.cuda.get_device_name(0)


so = lib.load_vilsolve()
lines = ["vscan_extract, %d warm calls per figure after %d warm-up calls; box %s (%s); commit %s" % (N, WARM, socket.gethostname(), device_name(), commit()),
         "wall = host clock around the call (upload, four kernels, read-back, copy-out), events off; kernel = HIP events, second pass",
         "no CPU timing baseline exists for this stage: the only CPU restatement is tests/scanreg_ref.py (Python, test infrastructure)"]
R, t = _rot(-0.01, 0.015, -0.7), np.array([-2.0, 1.5, 0.2])
for rings, lo, hi in ((16, -15.0, 15.0), (64, -24.9, 2.0)):
    raw = scanreg.make_raw_scan(R, t, seed=1, rings=rings, az=1800, lower=lo, upper=hi)
    reg = scanreg.ScanReg(so, scanreg.default_config(so, num_rings=rings, lower_bound_deg=lo, upper_bound_deg=hi), max_points=len(raw))
    for _ in range(WARM):
        f = reg.extract(raw)
    ts = []
    for _ in range(N):
        a = time.perf_counter(); reg.extract(raw); ts.append(time.perf_counter() - a)
    ts = 1e3 * np.array(ts)
    reg.profile_enable(True); reg.profile_read()
    for _ in range(N):
        reg.extract(raw)
    prof = reg.profile_read()
    reg.close()
    lines.append("%d rings x 1800 (%d points; %d sharp, %d less sharp, %d flat, %d less flat of %d before the filter): wall median %.3f ms, mean %.3f, p90 %.3f, min %.3f" %
                 (rings, len(raw), len(f.corner_sharp), len(f.corner_less_sharp), len(f.surf_flat), len(f.surf_less_flat), f.n_less_flat_raw,
                  np.median(ts), ts.mean(), np.percentile(ts, 90), ts.min()))
    for k in scanreg.KERNELS:
        n, ms = prof[k]
        lines.append("    %-18s %4d launches, %8.2f us per launch" % (k, n, 1e3 * ms / max(n, 1)))
    lines.append("    kernels together %8.2f us per scan" % (1e3 * sum(ms for _, ms in prof.values()) / N))
text = "\n".join(lines) + "\n"
print(text, end="")
os.makedirs(os.path.dirname(OUT), exist_ok=True)
open(OUT, "w").write(text)
