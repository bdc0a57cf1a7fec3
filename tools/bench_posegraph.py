"""Wall time and per-kernel HIP-event time of the pose-graph row (include/vilpgo.h): N in {500, 2000, 8000} poses on the tests' synthetic loop,
each with 0, 8 and 64 loop factors.  Per configuration:
  cold      vpgo_optimize from the drifted odometry values (the graph is rebuilt for every repeat; only the optimise is timed);
  per scan  one pose and its odometry factor are appended to the optimised graph, then vpgo_optimize from the previous solution;
  kernels   the split of one cold optimise from vpgo_profile_read;
  CPU       the same two cases for the NumPy restatement (tests/posegraph_ref.py: per-factor Python linearisation, scipy.sparse normal
            equations, SuperLU) on the host this runs on -- one run each, it is slow.
Written to profiles/posegraph.txt (OUT=<file> for another place) with the device, the host and the commit (VIL_COMMIT names it where the
sources are not a git checkout).

    python tools/bench_posegraph.py [repeats, default 5]

Every configuration runs in a child process of its own under a time limit of its own; one that fails or runs out of time ends the run, what
was measured until then is still written."""
import os
import platform
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import __graft_entry__ as g; g.load_package()
from mvil_fusion_amd import lib, posegraph
from _rowbench import commit, device_name, write
import posegraph_fixtures as pf
import posegraph_ref as pr

OUT = os.environ.get("OUT") or os.path.join(ROOT, "profiles", "posegraph.txt")
SIZES, LOOPS = (500, 2000, 8000), (0, 8, 64)


def host_name():
    try:
        return [l.split(":", 1)[1].strip() for l in open("/proc/cpuinfo") if l.startswith("model name")][0]
    except Exception:
        return platform.processor() or platform.machine()


def source_state():
    """the commit when the tree is a clean checkout of one; otherwise the parent commit, if known, and that the tree differs from it"""
    c = commit()
    if c.startswith("unknown"):
        return "sources not under version control"
    dirty = subprocess.run(["git", "-C", ROOT, "status", "--porcelain", "--untracked-files=no"], capture_output=True, text=True).stdout.strip()
    return "commit %s%s" % (c, " with uncommitted changes" if dirty else "")


def fixture(N, n_loops):
    """N + 1 poses are generated; the last one is the scan that is appended afterwards"""
    step = max(1, N // (2 * max(n_loops, 1)))
    loop_list = [(N - 2 - k * step, k * step) for k in range(n_loops)]
    fx = pf.make(N + 1, "none", positions=False, loop_list=loop_list)
    fac = pf.ordered_factors(fx)
    last = [f for f in fac if max(f[1], f[2]) == N]
    return fx, [f for f in fac if max(f[1], f[2]) < N], last


def build(graph, fx, fac, N):
    for T in fx["init"][:N]:
        graph.add_pose(T)
    for f in fac:
        pf.add_factor(graph, f)
    return graph


def ms(ts):
    ts = 1e3 * np.array(ts)
    return "median %.2f ms, min %.2f, max %.2f over %d" % (np.median(ts), ts.min(), ts.max(), len(ts))


def config(N, n_loops, repeats):
    so = lib.load_vilsolve()
    fx, fac, last = fixture(N, n_loops)
    new = lambda: posegraph.PoseGraph(so, max_poses=N + 2 * repeats + 8, max_factors=len(fac) + 2 * repeats + 8)
    lines, cold, scan = [], [], []
    sm = None
    for rep in range(repeats + 1):                                      # the first build and optimise warm the process up
        gr = build(new(), fx, fac, N)
        a = time.perf_counter(); sm = gr.optimize(); b = time.perf_counter()
        if rep:
            cold.append(b - a)
        if rep < repeats:
            gr.close()
    lines.append("N %d, %d loops (%d factors, %d separators, %d segments, reduced system %d wide)" % (N, n_loops, len(fac), sm.n_separators, sm.n_segments, sm.reduced_size))
    lines.append("  device cold      %s; %d iterations (%d accepted), termination %d, cost %.6g -> %.6g" % (ms(cold), sm.iterations, sm.accepted, sm.termination, sm.initial_cost, sm.final_cost))
    odo = last[0][3]
    sm2 = None
    for rep in range(repeats + 1):                                      # append a scan to the optimised graph, optimise; the first is the warm-up
        n = gr.size()[0]
        a = time.perf_counter()
        k = gr.add_pose(gr.poses(n - 1, 1)[0] @ odo); gr.add_between(n - 1, k, odo, pf.ODOM_VAR); sm2 = gr.optimize()
        b = time.perf_counter()
        if rep:
            scan.append(b - a)
    lines.append("  device per scan  %s; %d iterations, termination %d (read one pose back, append, optimise)" % (ms(scan), sm2.iterations, sm2.termination))
    gr.close()
    gr = build(new(), fx, fac, N)
    gr.profile_enable(True); gr.profile_read()
    gr.optimize()
    prof = gr.profile_read()
    gr.close()
    tot = sum(t for _, t in prof.values())
    lines.append("  kernels of one cold optimise (launches that returned at once after the finished flag included), %.2f ms together:" % tot)
    lines += ["    %-17s %5d launches %9.3f ms" % (k, n, t) for k, (n, t) in prof.items() if n]
    ref = build(pr.Graph(), fx, fac, N)
    a = time.perf_counter(); it, c0, c1, term = ref.optimize(); b = time.perf_counter()
    lines.append("  CPU cold         %.0f ms; %d iterations, termination %d, cost %.6g -> %.6g" % (1e3 * (b - a), it, term, c0, c1))
    a = time.perf_counter()
    k = ref.add_pose(ref.poses[-1] @ odo); ref.add_between(k - 1, k, odo, pf.ODOM_VAR); it, _, _, term = ref.optimize()
    b = time.perf_counter()
    lines.append("  CPU per scan     %.0f ms; %d iterations, termination %d" % (1e3 * (b - a), it, term))
    return lines


if __name__ == "__main__":
    if len(sys.argv) > 4 and sys.argv[1] == "--config":
        print("\n".join(config(int(sys.argv[2]), int(sys.argv[3]), int(sys.argv[4]))))
        sys.exit(0)
    repeats = max(2, int(sys.argv[1])) if len(sys.argv) > 1 else 5
    lines = ["pose-graph row (include/vilpgo.h); %s; host %s; %s" % (device_name(), host_name(), source_state()),
             "wall = host clock around vpgo_optimize (cold) or around read-back + two appends + vpgo_optimize (per scan), events off; kernels = HIP events, one more run",
             "default options: max_iterations 20, initial_lambda 1e-5, step_tolerance 1e-10, cost_tolerance 1e-12"]
    for N in SIZES:
        for n_loops in LOOPS:
            limit = 60 + N // 20
            try:
                p = subprocess.run([sys.executable, os.path.abspath(__file__), "--config", str(N), str(n_loops), str(repeats)], capture_output=True, text=True, timeout=limit)
            except subprocess.TimeoutExpired:
                lines.append("N %d, %d loops: no result within %d s; the run ends here" % (N, n_loops, limit))
                write(lines, OUT); sys.exit(1)
            if p.returncode != 0:
                lines.append("N %d, %d loops: exit status %d; the run ends here\n%s" % (N, n_loops, p.returncode, p.stderr[-1000:]))
                write(lines, OUT); sys.exit(1)
            lines.append(p.stdout.rstrip("\n"))
    write(lines, OUT)
