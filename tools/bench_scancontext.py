"""Per-call wall time and per-kernel HIP-event time of the Scan Context row (include/vilsc.h): vsc_push_scan for scans of 20 k and 100 k
points, vsc_detect in both modes against resident databases of 1 k and 10 k entries, written to profiles/scancontext.txt (OUT=<file> for
another place) with the device and the commit.

    python tools/bench_scancontext.py [calls, default 200]

Every step runs in a child process of its own under a time limit of its own; a step that fails or runs out of time ends the run, what
was measured until then is still written.  Wall time is taken with the profiling events off, kernel times in a second pass with them on.
There is no compiled CPU counterpart of this stage (Eigen, PCL and nanoflann are absent): the only CPU restatement is the Python one of
tests/scancontext_ref.py, which is test infrastructure and not a timing baseline, so no speed-up is claimed."""
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import __graft_entry__ as g; g.load_package()
from mvil_fusion_amd import lib, scancontext as sc
from _rowbench import WARM, commit, device_name, profiled, timed, write

OUT = os.environ.get("OUT") or os.path.join(ROOT, "profiles", "scancontext.txt")
STEPS = (("push", 20000, 120), ("push", 100000, 120), ("detect", 1000, 180), ("detect", 10000, 300))     # (what, size, time limit in s)


KERNEL_FMT = "    %-12s %5d launches, %8.2f us per launch"          # a line per kernel that ran: a push runs two of the six, a detect two or four


def step_push(n_points, calls):
    """A scan of n_points random points within 1.2 max_radius of the sensor (a part is skipped, as in a real scan)"""
    rng = np.random.default_rng(1)
    scan = rng.uniform(-68.0, 68.0, (n_points, 4)).astype(np.float32); scan[:, 2] = rng.uniform(-2.0, 8.0, n_points)
    ctx = sc.ScanContext(lib.load_vilsolve(), max_entries=2 * (calls + WARM), max_points=n_points)
    _, wall = timed(lambda: ctx.push_scan(scan), calls)
    ctx.reset()
    kernels = profiled(ctx, lambda: ctx.push_scan(scan), calls, fmt=KERNEL_FMT, idle=False)
    occupied = int((ctx.read_entry(0)[0] != 0).sum())
    ctx.close()
    return ["vsc_push_scan, %d points (%d of 1200 bins occupied): %s" % (n_points, occupied, wall)] + kernels


def step_detect(n_entries, calls):
    """A database of n_entries random descriptors (a tenth of them shifted copies of earlier ones); the query is a shifted copy too"""
    rng = np.random.default_rng(2)
    ctx = sc.ScanContext(lib.load_vilsolve(), max_entries=n_entries + 1, max_points=16)
    base = [np.where(rng.random((20, 60)) < 0.5, rng.uniform(0.0, 6.0, (20, 60)), 0.0).astype(np.float32) for _ in range(64)]
    t0 = time.perf_counter()
    for i in range(n_entries):
        ctx.push_descriptor(np.roll(base[int(rng.integers(0, 64))], int(rng.integers(0, 60)), axis=1) if i % 10 == 0 else rng.uniform(0.0, 6.0, (20, 60)).astype(np.float32))
    fill = time.perf_counter() - t0
    ctx.push_descriptor(np.roll(base[3], 17, axis=1))
    lines = ["database of %d entries (filled through vsc_push_descriptor in %.2f s)" % (n_entries, fill)]
    for mode, name in ((sc.MODE_REFERENCE, "REFERENCE"), (sc.MODE_EXHAUSTIVE, "EXHAUSTIVE")):
        r, wall = timed(lambda: ctx.detect(mode), calls)
        kernels = profiled(ctx, lambda: ctx.detect(mode), calls, fmt=KERNEL_FMT, idle=False)
        ctx.profile_enable(False)
        lines.append("vsc_detect %s, %d searched (loop_id %d, min_dist %.3g, nn_align %d): %s" % (name, r.n_searched, r.loop_id, r.min_dist, r.nn_align, wall))
        lines += kernels
    ctx.close()
    return lines


if __name__ == "__main__":
    if len(sys.argv) > 3 and sys.argv[1] == "--step":
        fn = step_push if sys.argv[2] == "push" else step_detect
        print("\n".join(fn(int(sys.argv[3]), int(sys.argv[4]))))
        sys.exit(0)
    calls = max(50, int(sys.argv[1])) if len(sys.argv) > 1 else 200
    lines = ["Scan Context row (include/vilsc.h), %d warm calls per figure after %d warm-up calls; %s; commit %s" % (calls, WARM, device_name(), commit()),
             "wall = host clock around the call, events off; kernel = HIP events, second pass",
             "no CPU timing baseline exists for this stage: the only CPU restatement is tests/scancontext_ref.py (Python, test infrastructure)"]
    for what, size, limit in STEPS:
        try:
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--step", what, str(size), str(calls)], capture_output=True, text=True, timeout=limit)
        except subprocess.TimeoutExpired:
            lines.append("%s %d: no result within %d s; the run ends here" % (what, size, limit))
            break
        if p.returncode != 0:
            lines.append("%s %d: exit status %d; the run ends here\n%s" % (what, size, p.returncode, p.stderr[-1000:]))
            break
        lines.append(p.stdout.rstrip("\n"))
    write(lines, OUT)
