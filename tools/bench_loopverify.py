"""Per-call wall time and per-kernel HIP-event time of the fitness / loop-verification row (include/villoop.h): vloop_score on the
synthetic scan pair at 2.4 k, 14.4 k and 57.6 k points per scan, through the grid and through the exhaustive search, at the pair's true
transform and at a 50 m offset (every query then ends in the grid search's exhaustive fallback), and vloop_verify over 1 and 8
candidates, written to profiles/loopverify.txt (OUT=<file> for another place) with the device and the commit.

    python tools/bench_loopverify.py [calls, default 100]

Every step runs in a child process of its own under a time limit of its own; a step that fails or runs out of time ends the run, what
was measured until then is still written.  Wall time is taken with the profiling events off, kernel times in a second pass with them on.
There is no compiled CPU counterpart of this stage (PCL is absent): the only CPU restatement is the NumPy one of tests/loopverify_ref.py,
which is test infrastructure and not a timing baseline, so no speed-up is claimed."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import __graft_entry__ as g; g.load_package()
from mvil_fusion_amd import lib, loopverify as lv, vgicp
from _rowbench import WARM, commit, device_name, profiled, timed, write

OUT = os.environ.get("OUT") or os.path.join(ROOT, "profiles", "loopverify.txt")
STEPS = (("score", 8, 300, 120), ("score", 16, 900, 180), ("score", 64, 900, 300), ("verify", 8, 300, 240))     # (what, rings, azimuths, time limit in s)
KERNEL_FMT = "    %-14s %5d launches, %9.2f us per launch"


def step_score(rings, az, calls):
    tx, _, sx, _, T_true = vgicp.make_pair(0, rings=rings, az=az)
    n = len(sx)
    far = T_true.copy(); far[0, 3] += 50.0
    ctx = lv.LoopVerify(lib.load_vilsolve(), max_points=n)
    ctx.set_source(sx)
    lines = []
    for path, min_points in (("grid, cell 0.5 m", 0), ("exhaustive", 1 << 30)):
        ctx.set_grid(min_points, 0.5); ctx.set_target(tx)
        for what, T in (("true transform", T_true), ("50 m offset", far)):
            k = calls if n < 20000 or what == "true transform" and min_points == 0 else max(10, calls // 5)
            (s, used), wall = timed(lambda: ctx.score(T), k)
            kernels = profiled(ctx, lambda: ctx.score(T), k, fmt=KERNEL_FMT, idle=False)
            ctx.profile_enable(False)
            lines.append("vloop_score, %d x %d points, %s, %s (score %.6g, %d used), %d calls: %s" % (n, len(tx), path, what, s, used, k, wall))
            lines += kernels
    T8 = np.tile(T_true, (8, 1, 1))
    ctx.set_grid(1024, 0.5); ctx.set_target(tx)
    _, wall = timed(lambda: ctx.score(T8), calls)
    lines.append("vloop_score, %d points, 8 transforms in one call (default path): %s" % (n, wall))
    ctx.close()
    return lines


def step_verify(rings, az, calls):
    so = lib.load_vilsolve()
    tx, _, sx, _, T_true = vgicp.make_pair(0, rings=rings, az=az)
    ctx = lv.LoopVerify(so, max_points=len(sx)); reg = vgicp.Vgicp(so)
    opts = lv.default_options(so)
    lines = []
    for n_cand in (1, 8):
        cands = [(tx, np.eye(4))] * n_cand
        k = max(10, calls // (2 * n_cand))
        (best, per), wall = timed(lambda: ctx.verify(reg, sx, cands, opts), k)
        lines.append("vloop_verify, query %d points, %d candidate(s) of %d points (winner %d, fitness %.6g, %d iterations), %d calls: %s" %
                     (len(sx), n_cand, len(tx), best.index, best.fitness, per[0].iterations, k, wall))
    lines.append("    (a candidate costs vgicp_set_target with its covariance estimate and host-side voxel map, vloop_set_target, vgicp_align and one vloop_score)")
    ctx.close(); reg.close()
    return lines


if __name__ == "__main__":
    if len(sys.argv) > 4 and sys.argv[1] == "--step":
        fn = step_score if sys.argv[2] == "score" else step_verify
        print("\n".join(fn(int(sys.argv[3]), int(sys.argv[4]), int(sys.argv[5]))))
        sys.exit(0)
    calls = max(20, int(sys.argv[1])) if len(sys.argv) > 1 else 100
    lines = ["fitness / loop-verification row (include/villoop.h), each figure over the calls its line names, after %d warm-up calls; %s; commit %s" % (WARM, device_name(), commit()),
             "wall = host clock around the call, events off; kernel = HIP events, second pass",
             "k_loop_grid is one wave per query; a one-lane-per-query grid search was not built, so there is no comparison of the two",
             "no CPU timing baseline exists for this stage: the only CPU restatement is tests/loopverify_ref.py (NumPy, test infrastructure)"]
    for what, rings, az, limit in STEPS:
        try:
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--step", what, str(rings), str(az), str(calls)], capture_output=True, text=True, timeout=limit)
        except subprocess.TimeoutExpired:
            lines.append("%s %d x %d: no result within %d s; the run ends here" % (what, rings, az, limit))
            break
        if p.returncode != 0:
            lines.append("%s %d x %d: exit status %d; the run ends here\n%s" % (what, rings, az, p.returncode, p.stderr[-1000:]))
            break
        lines.append(p.stdout.rstrip("\n"))
    write(lines, OUT)
