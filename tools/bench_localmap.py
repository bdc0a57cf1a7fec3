"""Wall time, per-kernel HIP-event time, bytes moved and host waits of vlmap_push_scan (include/villmap.h) in the mapping node's steady
state, written to profiles/localmap.txt (OUT=<file> for another place) with the device and the commit.

    python tools/bench_localmap.py

The scan is the feature clouds of a 16 x 1800-style scan (800 corner + 6000 surf points, the sizes of `bench.py --mapreg`) against a
settled local map of that bench's size (8000 + 60000 points before the cubes' filters).  Medians after a warm-up.  In the same run, on the
same inputs: the same work as the chain of the library's public calls (vcloud_filter, vmap_set_map, vmap_align, vcloud_filter per valid
cube) with the cube bookkeeping in NumPy -- its wall time, and the time inside its device calls alone.  The reference's own host code has
no compiled implementation here (PCL is absent), so nothing below is a speed-up claim against it.  Last: the refilter at its worst case,
every point of a cube in one voxel, where one thread adds the whole cube (the sequential float sum is the contract)."""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import __graft_entry__ as g; g.load_package()
from mvil_fusion_amd import cloud, lib, localmap, mapreg
from mvil_fusion_amd.vgicp import _rot
from _rowbench import commit, device_name, write

OUT = os.environ.get("OUT") or os.path.join(ROOT, "profiles", "localmap.txt")
WARM, REPS = 5, 15
F = np.float32
CFG = dict(max_scan_points=8192, max_map_points=1 << 18, publish_first_frame=1 << 30, publish_frames=1 << 30, publish_distance=1e9)
SIZE = np.array([10.0, 10.0, 5.0]); CEN = np.array([5, 5, 3]); DIM = np.array([11, 11, 7])


def cube_of(xyz):
    """the header's steps 2 / 6 for n x 3 coordinates: cube index, -1 outside the array"""
    s = np.asarray(xyz, np.float64)
    k = np.trunc(s / SIZE).astype(np.int64) - (s < 0) + CEN
    ok = ((k >= 0) & (k < DIM)).all(axis=1)
    return np.where(ok, k[:, 0] + 11 * k[:, 1] + 121 * k[:, 2], -1)


def valid_cubes(t):
    c = cube_of(np.asarray(t).reshape(1, 3))[0]
    ci, cj, ck = c % 11, (c // 11) % 11, c // 121
    return [i + 11 * j + 121 * k for i in range(ci - 2, ci + 3) for j in range(cj - 2, cj + 3) for k in range(ck - 1, ck + 2) if 0 <= i < 11 and 0 <= j < 11 and 0 <= k < 7]


def to_map(q, t, p):
    x, y, z, w = q
    R = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)], [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                  [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])
    out = p.copy()
    out[:, :3] = (p[:, :3].astype(np.float64) @ R.T + t).astype(F)
    return out


class Chain:
    """The same scan through the public calls; the cubes are NumPy arrays on the host."""

    def __init__(self, so, be, cubes):
        self.be, self.reg, self.filt = be, mapreg.MapReg(so), cloud.DepthCloud(so, max_scan_points=1 << 16, max_scans=1)
        self.cubes = [dict(c) for c in cubes]
        self.dev = 0.0; self.up = 0; self.down = 0; self.waits = 0

    def call(self, fn, *a, up=0, waits=1):
        t0 = time.perf_counter(); r = fn(*a); self.dev += time.perf_counter() - t0
        self.up += up; self.waits += waits
        return r

    def filter(self, pts, leaf):
        out = self.call(self.filt.filter, pts, leaf, 512, up=pts.nbytes, waits=2)                  # its header, then its points
        self.down += 64 + out.nbytes
        return out

    def push(self, corner, surf, q, t):
        self.dev = 0.0; self.up = self.down = self.waits = 0
        valid = valid_cubes(t)
        fm = [np.concatenate([self.cubes[cls].get(e, np.zeros((0, 4), F)) for e in valid]) for cls in range(2)]
        self.call(self.reg.set_map, fm[0], fm[1], up=fm[0].nbytes + fm[1].nbytes, waits=3)         # two grid builds (a read-back each, more while the cell size adapts) and the end
        stack = [self.filter(corner, 0.2), self.filter(surf, 0.4)]
        q2, t2, sm = self.call(self.reg.align, self.be.ctx, stack[0], stack[1], q, t, up=stack[0].nbytes + stack[1].nbytes, waits=1)
        self.down += 176
        for cls in range(2):
            placed = to_map(q2, t2, stack[cls]); key = cube_of(placed[:, :3])
            for e in np.unique(key[key >= 0]):
                self.cubes[cls][e] = np.concatenate([self.cubes[cls].get(e, np.zeros((0, 4), F)), placed[key == e]])
        for e in valid:
            for cls, leaf in ((0, 0.2), (1, 0.4)):
                if len(self.cubes[cls].get(e, ())):
                    self.cubes[cls][e] = self.filter(self.cubes[cls][e], leaf)
        return q2, t2

    def close(self):
        self.reg.close(); self.filt.close()


def med(ts):
    ts = np.asarray(ts)
    return "median %8.3f ms, min %8.3f, max %8.3f" % (np.median(ts), ts.min(), ts.max())


def main():
    so = lib.load_vilsolve(); be = lib.open_vilsolve(device=0)
    cm, sm = mapreg.make_map(seed=20240607, n_surf=60000, n_corner=8000)
    R, t = _rot(0.01, -0.015, 0.5), np.array([1.5, -1.0, 0.25])
    sc, ss = mapreg.make_scan(cm, sm, R, t, seed=11, n_surf=6000, n_corner=800)
    q0 = mapreg.quat_from_R(R @ _rot(0.004, -0.003, 0.008)); t0 = t + np.array([0.05, -0.04, 0.03])
    lm = localmap.LocalMap(so, **CFG)
    for cls, M in ((0, cm), (1, sm)):                                                              # the map into its cubes, raw; the first push filters the valid ones
        key = cube_of(M[:, :3])
        for e in np.unique(key[key >= 0]):
            lm.debug_write_cube(cls, int(e), M[key == e])
    empty = np.zeros((0, 4), F)
    s = lm.push_scan(be.ctx, empty, empty, q0, t0)
    for _ in range(WARM):
        s = lm.push_scan(be.ctx, sc, ss, q0, t0)
    settled = [{e: lm.read_cube(cls, e) for e in range(localmap.CUBES) if len(lm.read_cube(cls, e))} for cls in range(2)]
    ts = []
    for _ in range(REPS):
        a = time.perf_counter(); s = lm.push_scan(be.ctx, sc, ss, q0, t0); ts.append(1e3 * (time.perf_counter() - a))
    occupied = [sum(1 for e in valid_cubes(t0) if len(lm.read_cube(cls, e))) for cls in range(2)]
    lines = ["vlmap_push_scan, %s, commit %s" % (device_name(), commit()),
             "scan %d corner + %d surf feature points -> stacks %d + %d; map %d + %d points in all cubes, from-map %d + %d; %d + %d of the 75 valid cubes hold points; aligned %d, "
             "%d edge + %d plane factors" % (len(sc), len(ss), s.n_corner_stack, s.n_surf_stack, s.n_corner_map, s.n_surf_map, s.n_corner_from_map, s.n_surf_from_map, occupied[0],
                                             occupied[1], s.aligned, s.align.n_edge, s.align.n_plane),
             "medians of %d pushes after %d warm-up pushes; the map is settled (every push appends the scan and the refilter merges it away)" % (REPS, WARM),
             "", "resident call          wall " + med(ts)]
    up = 4 * (4 * localmap.CUBES + 76 * 3) + 16 * (len(sc) + len(ss)) + 8
    down = 64 + 4 * (16 + 24 + 4 * localmap.CUBES) + 176
    lines += ["    bytes up %d (the two feature clouds, the cube table), down %d (the stacks' counts, the new table, the alignment's record)" % (up, down),
              "    host waits: 1 (the stacks' counts) + vmap_set_map's (2 grid builds with a read-back each, and its end) + vmap_align's 1 + 1 (the table)"]
    lm.profile_enable(True); lm.profile_read()
    for _ in range(REPS):
        lm.push_scan(be.ctx, sc, ss, q0, t0)
    prof = lm.profile_read(); lm.profile_enable(False)
    lines += ["    %-18s %4d launches, %8.2f us per launch" % (k, n, 1e3 * ms / max(n, 1)) for k, (n, ms) in prof.items()]
    lines += ["    this row's kernels together %8.2f us per push (the stacks' filter A and the registration are the cloud and map rows' kernels: profiles/cloud.txt, bench.py --mapreg)" %
              (1e3 * sum(ms for _, ms in prof.values()) / REPS)]

    ch = Chain(so, be, settled)
    for _ in range(WARM):
        ch.cubes = [dict(c) for c in settled]; ch.push(sc, ss, q0, t0)
    tw, td = [], []
    for _ in range(REPS):
        ch.cubes = [dict(c) for c in settled]
        a = time.perf_counter(); ch.push(sc, ss, q0, t0); tw.append(1e3 * (time.perf_counter() - a)); td.append(1e3 * ch.dev)
    lines += ["", "chain of public calls  wall " + med(tw), "    inside its device calls  " + med(td),
              "    bytes up %d (the from-map clouds, the scans twice, every valid cube), down %d (the stacks, every valid cube); host waits %d" % (ch.up, ch.down, ch.waits)]
    ch.close()
    r, c = np.median(ts), np.median(td)
    lines += ["", "the resident call takes %.2f x the chain's device calls alone and %.2f x the chain's wall time" % (r / c, r / np.median(tw))]

    lines += ["", "refilter, one cube of n points (k_lmap_refilter, HIP events, one push with empty scans each)"]
    rng = np.random.default_rng(1)
    for n in (1024, 8192, 65536):
        row = "    n %6d:" % n
        for name, pts in (("all in ONE voxel", np.concatenate([rng.uniform(1.001, 1.199, (n, 3)), np.ones((n, 1))], axis=1).astype(F)),
                          ("spread over the cube", np.concatenate([rng.uniform(0.0, 10.0, (n, 3)) * [1, 1, 0.5], np.ones((n, 1))], axis=1).astype(F))):
            lm.reset(); lm.debug_write_cube(0, 5 + 55 + 363, pts)
            lm.profile_enable(True); lm.profile_read()
            s1 = lm.push_scan(be.ctx, empty, empty, np.array([0.0, 0.0, 0.0, 1.0]), np.zeros(3))
            ms = lm.profile_read()["k_lmap_refilter"][1]; lm.profile_enable(False)
            row += "  %s %9.1f us (-> %d points)" % (name, 1e3 * ms, s1.n_corner_map)
        lines.append(row)
    lm.close(); be.close()
    write(lines, OUT)


if __name__ == "__main__":
    main()
