"""Wall time and per-kernel HIP-event time of the global-map row (include/vilgmap.h).
  per scan  one cycle of the mapping node on a map of 100 k, 1 M and 4 M points: vgmap_reference for a 4 k-point query (the scan after its
            0.3 m filter) + vgmap_insert of the 16 k-point scan, in both variants: OcTree (0.05 m map, radius mode) and IkdTree (no thinning,
            kNN mode).  The insert changes the map, so every cycle rebuilds the search grid; its share is printed.
  rebuild   vgmap_rebuild of 500 and 2000 keyed scans of 16 k points at 0.05 m.
  CPU       the same work by the NumPy restatement with scipy's cKDTree as its search structure (a tree built per cycle, query_ball_point /
            query, np.unique for the voxels) on the host this runs on, one run each.  PCL is not on these machines: this is the tests'
            restatement with a tree, NOT the reference's octree / ikd-Tree and no fair CPU opponent.
Medians of 5 after a warm-up.  Written to profiles/globalmap.txt (OUT=<file> for another place).

    python tools/bench_globalmap.py [repeats, default 5]

Every configuration runs in a child process of its own under a time limit of its own; one that fails or runs out of time ends the run, what
was measured until then is still written."""
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import __graft_entry__ as g; g.load_package()
from mvil_fusion_amd import globalmap, lib
from _rowbench import device_name, write
from bench_posegraph import host_name, source_state
import globalmap_ref as gr
from scipy.spatial import cKDTree

OUT = os.environ.get("OUT") or os.path.join(ROOT, "profiles", "globalmap.txt")
MAPS, KEYED = (100_000, 1_000_000, 4_000_000), (500, 2000)
SCAN, QUERY, CHUNK = 16384, 4096, 1 << 17
F32 = np.float32


def world(n):
    """n points that all survive at 0.05 m: a floor sampled every 0.06 m, with a little height noise"""
    side = int(np.ceil(np.sqrt(n)))
    i = np.arange(n)
    rng = np.random.default_rng(1)
    return np.stack([0.06 * (i % side) + 0.03, 0.06 * (i // side) + 0.03, rng.uniform(0.0, 0.04, n)], axis=1).astype(F32), 0.06 * side


def scan_at(rng):
    """a 16 k-point scan of the floor and of things standing on it within 8 m of the sensor, in the sensor frame"""
    r = 8.0 * np.sqrt(rng.uniform(0, 1, SCAN)); a = rng.uniform(0, 2 * np.pi, SCAN)
    return np.stack([r * np.cos(a), r * np.sin(a), np.where(rng.uniform(size=SCAN) < 0.8, rng.uniform(0.0, 0.04, SCAN), rng.uniform(0.0, 2.0, SCAN))], axis=1).astype(F32)


def ms(ts):
    ts = 1e3 * np.array(ts)
    return "median %.2f ms, min %.2f, max %.2f over %d" % (np.median(ts), ts.min(), ts.max(), len(ts))


def cpu_cycle(points, keys, q, s, T, mode, res):
    """the restatement's steps with a kd-tree: (seconds, n_ref, new points)"""
    a = time.perf_counter()
    tree = cKDTree(points)
    qw = gr.transform(T, q)
    if mode == "radius":
        u = np.unique(np.concatenate(tree.query_ball_point(qw, 0.5, return_sorted=False)).astype(np.int64))
        _, first = np.unique(gr.pack(gr.voxel(points[u], 0.3)), return_index=True)
        n_ref = len(first)
    else:
        d, j = tree.query(qw, k=5)
        n_ref = int((d * d <= 1.5).sum())
    sw = gr.transform(T, s)
    if res > 0:
        k = gr.pack(gr.voxel(sw, res))
        _, first = np.unique(k, return_index=True)
        first = first[~np.isin(k[first], keys)]
        sw = sw[np.sort(first)]
    return time.perf_counter() - a, n_ref, len(sw)


def per_scan(n_map, mode, repeats):
    so = lib.load_vilsolve()
    res = 0.05 if mode == "radius" else 0.0
    pts, side = world(n_map)
    gm = globalmap.GlobalMap(so, max_map_points=n_map + (2 * repeats + 4) * SCAN, max_scan_points=CHUNK, max_keys=1, max_keyed_points=1, max_ref_points=1 << 18, map_resolution=res)
    for a in range(0, n_map, CHUNK):
        gm.insert(pts[a:a + CHUNK], np.eye(4))
    rng = np.random.default_rng(2)
    cyc, refs, ins, n_ref = [], [], [], 0
    T = None
    for rep in range(2 * repeats + 1):                                  # one warm-up cycle, `repeats` timed ones, `repeats` with the kernel events on
        T = gr.pose(*rng.uniform(side / 3, 2 * side / 3, 2), 0.0, rng.uniform(0, 6.28))              # the 16 m scan disc lies inside the map for all but the smallest
        s = scan_at(rng); q = s[::SCAN // QUERY]
        if rep == repeats + 1:
            gm.profile_enable(True); gm.profile_read()
        a = time.perf_counter(); x, i = gm.reference(q, T, T_out=np.linalg.inv(T), mode=mode); b = time.perf_counter(); gm.insert(s, T); c = time.perf_counter()
        if 1 <= rep <= repeats:
            cyc.append(c - a); refs.append(b - a); ins.append(c - b)
        n_ref = len(i)
    prof = gm.profile_read()
    tot = sum(t for _, t in prof.values())
    n_now = gm.size()[0]
    lines = ["%s variant (%s), map of %d points (%d after the cycles), scan %d, query %d, %d reference points" %
             ("OcTree" if mode == "radius" else "IkdTree", "0.05 m, radius 0.5, thinned to 0.3 m" if mode == "radius" else "no thinning, k 5, max_dist 1.5", n_map, n_now, SCAN, QUERY, n_ref),
             "  device cycle     %s" % ms(cyc), "    reference      %s" % ms(refs), "    insert         %s" % ms(ins),
             "  kernels of %d cycles, %.3f ms per cycle together; the search grid's rebuild is %.3f ms per cycle = %.0f %% of the kernel time, %.0f %% of the cycle's wall time" %
             (repeats, tot / repeats, prof["grid"][1] / repeats, 100 * prof["grid"][1] / tot, 100 * (prof["grid"][1] / repeats) / (1e3 * np.median(cyc)))]
    lines += ["    %-15s %3d launches %9.3f ms per cycle" % (k, n, t / repeats) for k, (n, t) in prof.items() if n]
    allp = gm.points()
    gm.close()
    keys = gr.pack(gr.voxel(allp, 0.05)) if res > 0 else None
    t, nr, _ = cpu_cycle(allp, keys, q, s, T, mode, res)
    lines.append("  CPU restatement with cKDTree, one cycle: %.0f ms (%d reference points)" % (1e3 * t, nr))
    return lines


def rebuild(n_keys, repeats):
    so = lib.load_vilsolve()
    total = n_keys * SCAN
    gm = globalmap.GlobalMap(so, max_map_points=total, max_scan_points=SCAN, max_keys=n_keys, max_keyed_points=total, max_ref_points=1, map_resolution=0.05)
    rng = np.random.default_rng(3)
    scans = [scan_at(rng) for _ in range(8)]
    for k in range(n_keys):
        gm.add_scan(k, scans[k % 8])
    poses = np.array([gr.pose(0.5 * k, 3.0 * np.sin(0.01 * k), 0.0, 0.002 * k) for k in range(n_keys)])
    keys = np.arange(n_keys)
    ts = []
    for rep in range(2 * repeats + 1):
        if rep == repeats + 1:
            gm.profile_enable(True); gm.profile_read()
        P = poses.copy(); P[:, 0, 3] += 1e-3 * rep                      # corrected poses differ from the last ones
        a = time.perf_counter(); gm.rebuild(keys, P); b = time.perf_counter()
        if 1 <= rep <= repeats:
            ts.append(b - a)
    prof = gm.profile_read()
    n_map = gm.size()[0]
    gm.close()
    lines = ["rebuild of %d keyed scans (%d points) at 0.05 m -> a map of %d points" % (n_keys, total, n_map), "  device           %s" % ms(ts),
             "  kernels, %.3f ms per rebuild together:" % (sum(t for _, t in prof.values()) / repeats)]
    lines += ["    %-15s %3d launches %9.3f ms per rebuild" % (k, n, t / repeats) for k, (n, t) in prof.items() if n]
    a = time.perf_counter()
    q = np.concatenate([gr.transform(P[k], scans[k % 8]) for k in range(n_keys)])
    _, first = np.unique(gr.pack(gr.voxel(q, 0.05)), return_index=True)
    m = q[np.sort(first)]
    lines.append("  CPU restatement (NumPy transform + np.unique), one run: %.0f ms (%d points)" % (1e3 * (time.perf_counter() - a), len(m)))
    return lines


if __name__ == "__main__":
    if len(sys.argv) > 4 and sys.argv[1] == "--per-scan":
        print("\n".join(per_scan(int(sys.argv[2]), sys.argv[3], int(sys.argv[4]))))
        sys.exit(0)
    if len(sys.argv) > 3 and sys.argv[1] == "--rebuild":
        print("\n".join(rebuild(int(sys.argv[2]), int(sys.argv[3]))))
        sys.exit(0)
    repeats = max(2, int(sys.argv[1])) if len(sys.argv) > 1 else 5
    lines = ["global-map row (include/vilgmap.h); %s; host %s; %s" % (device_name(), host_name(), source_state()),
             "wall = host clock around vgmap_reference + vgmap_insert (cycle) or vgmap_rebuild, events off; kernels = HIP events, %d more runs" % repeats,
             "the CPU figure is the tests' NumPy restatement with scipy's cKDTree, not the reference's PCL octree / ikd-Tree: no fair opponent"]
    jobs = [(["--per-scan", str(n), mode, str(repeats)], 60 + n // 20000) for n in MAPS for mode in ("radius", "knn")] + [(["--rebuild", str(k), str(repeats)], 90 + k // 10) for k in KEYED]
    for args, limit in jobs:
        print("running", " ".join(args), file=sys.stderr, flush=True)
        try:
            p = subprocess.run([sys.executable, os.path.abspath(__file__)] + args, capture_output=True, text=True, timeout=limit)
        except subprocess.TimeoutExpired:
            lines.append("%s: no result within %d s; the run ends here" % (" ".join(args), limit))
            write(lines, OUT); sys.exit(1)
        if p.returncode != 0:
            lines.append("%s: exit status %d; the run ends here\n%s" % (" ".join(args), p.returncode, p.stderr[-1000:]))
            write(lines, OUT); sys.exit(1)
        lines.append(p.stdout.rstrip("\n"))
    write(lines, OUT)
