"""Per-image host time of the device-resident feature tracker (include/vilfeat.h) against the chain of this library's own separate calls.
  workload  640 x 480, max_level 3, MAX_CNT 150, MIN_DIST 30, 1000 hypotheses, equalize 1 (tiles 8 x 8, clip limit 3.0), the reference's
            camera; sequences of SEQ images of mvil-fusion_amd/track.py's synthetic sequence with noise sigma 2, every image published.
  two paths on the same images in the same run, alternating sequence by sequence:
    fused   vfeat_read_image per image;
    chain   tests/feat_ref.py over the device wrappers: vclahe_push, vtrack_track, vepi_reject, vtrack_detect, vepi_undistort per image
            with the bookkeeping in NumPy between them.  Its yardstick is the sum of the host-clock times INSIDE its ctypes calls, so the
            Python glue between the calls is not charged to it; its whole wall time is given as well.
  The first image of a sequence (no points yet; the chain pushes it twice after a reset) is not timed.  Medians over the timed images of
  all sequences after one warm-up sequence per path.  The new kernels' HIP-event times come from a second pass.  host_waits / bytes per
  image: the fused path's are its summary's, the chain's are counted from its call pattern (the sizes of its copies and of what its kernels
  write to pinned memory).  There is no compiled CPU opponent on these machines (no OpenCV): the only claim is "against the chain of this
  library's own calls".  Written to profiles/feat.txt (OUT=<file> for another place).

    python tools/bench_feat.py [sequences, default 6]"""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import __graft_entry__ as g; g.load_package()
from mvil_fusion_amd import epipolar, feat, lib, track
from _rowbench import device_name, write
from bench_posegraph import host_name, source_state
import feat_ref as fr

OUT = os.environ.get("OUT") or os.path.join(ROOT, "profiles", "feat.txt")
W, H, LEVELS, MAX_CNT, MIN_DIST, ITERS, SEQ = 640, 480, 3, 150, 30, 1000, 8
CAM = {k: epipolar.REFERENCE_CAMERA[k] for k in ("fx", "fy", "cx", "cy", "k1", "k2", "p1", "p2", "focal")}


class Meter:
    """wraps a row's _call: the host-clock time inside the ctypes calls, the waits and the bytes of the call pattern"""

    def __init__(self):
        self.zero()

    def zero(self):
        self.inside, self.waits, self.up, self.down = 0.0, 0, 0, 0

    def attach(self, row):
        inner = row._call

        def timed(name, *args):
            a = time.perf_counter()
            try:
                return inner(name, *args)
            finally:
                self.inside += time.perf_counter() - a
                self.account(name, args)
        row._call = timed

    def account(self, name, args):
        n = args[0].value if args and hasattr(args[0], "value") and name in ("track", "reject", "detect", "undistort") else 0
        if name == "push":                                  # vclahe_push: the raw image up, one synchronisation
            self.waits += 1; self.up += W * H
        elif name == "track" and n:                         # points up, forw_xy and status back
            self.waits += 1; self.up += 8 * n; self.down += 9 * n
        elif name == "reject" and n >= 8:                   # both point sets up; the kernel writes every count and inlier row to pinned memory
            self.waits += 1; self.up += 16 * n; self.down += ITERS * (4 + 8 * ((MAX_CNT + 63) // 64))
        elif name == "detect":                              # tracks up; the counters, kept (its whole field) and the picks back
            self.waits += 1; self.up += 8 * n; self.down += 64 + ((MAX_CNT + 15) // 16) * 16 + 8 * MAX_CNT
        elif name == "undistort" and n:                     # points and ids up, un and vel back
            self.waits += 1; self.up += 12 * n; self.down += 16 * n


def same(a, b):
    return all(a[0][k].tobytes() == b[0][k].tobytes() for k in fr.CHANNELS) and all(x.tobytes() == y.tobytes() for x, y in zip(a[1], b[1]))


if __name__ == "__main__":
    n_seq = max(2, int(sys.argv[1])) if len(sys.argv) > 1 else 6
    so = lib.load_vilsolve()
    ft = feat.FeatureTracker(so, W, H, CAM, max_level=LEVELS, max_iters=ITERS, equalize=True, max_cnt=MAX_CNT, min_dist=MIN_DIST)
    backend = fr.DeviceBackend(so, W, H, CAM, LEVELS, MAX_CNT, max_iters=ITERS, equalize=True)
    chain = fr.FeatRef(backend, MAX_CNT, MIN_DIST)
    meter = Meter()
    for row in (backend.t, backend.e, backend.c):
        meter.attach(row)
    fused_ms, chain_in_ms, chain_wall_ms, f_waits, f_up, f_down, c_waits, c_up, c_down, equal, images = [], [], [], [], [], [], [], [], [], True, 0
    for s in range(1 + n_seq):                              # sequence 0 warms both paths up
        imgs, _ = track.sequence(H, W, SEQ, seed=10 + s, noise=2.0)
        ft.reset(); chain.reset()
        got = []
        for k, img in enumerate(imgs):
            a = time.perf_counter(); m, sm = ft.read_image(img, 0.1 * k, True, 1000 + k); b = time.perf_counter()
            got.append((m, ft.debug_state(), ft.debug_un_vel()))
            if s and k:
                fused_ms.append(1e3 * (b - a)); f_waits.append(sm.host_waits); f_up.append(sm.bytes_up); f_down.append(sm.bytes_down)
        for k, img in enumerate(imgs):
            meter.zero()
            a = time.perf_counter(); m, _ = chain.read_image(img, 0.1 * k, True, 1000 + k); b = time.perf_counter()
            if s and k:
                chain_in_ms.append(1e3 * meter.inside); chain_wall_ms.append(1e3 * (b - a)); c_waits.append(meter.waits); c_up.append(meter.up); c_down.append(meter.down)
                images += 1
                equal &= same(got[k][:2], (m, (chain.pts, chain.ids, chain.cnt))) and got[k][2][0].tobytes() == chain.un.tobytes() and got[k][2][1].tobytes() == chain.vel.tobytes()
    ft.profile_enable(True); ft.profile_read()              # second pass: the new kernels' event times
    imgs, _ = track.sequence(H, W, SEQ, seed=10, noise=2.0)
    ft.reset()
    for k, img in enumerate(imgs):
        ft.read_image(img, 0.1 * k, True, 1000 + k)
    prof = ft.profile_read(); ft.profile_enable(False)
    med = lambda v: float(np.median(v))
    lines = ["The device-resident feature tracker (include/vilfeat.h) against the chain of separate row calls; %s; host %s; %s" % (device_name(), host_name(), source_state()),
             "%d x %d, max_level %d, MAX_CNT %d, MIN_DIST %d, %d hypotheses, equalize 1; %d sequences of %d images after one warm-up sequence, the first image of a" %
             (W, H, LEVELS, MAX_CNT, MIN_DIST, ITERS, n_seq, SEQ),
             "sequence not timed: %d timed images per path, every image published.  Host clock, medians.  No compiled CPU opponent exists on these machines (no" % images,
             "OpenCV): the only comparison is against the chain of this library's own calls.",
             "  fused   vfeat_read_image                         median %7.3f ms per image (min %7.3f, max %7.3f)" % (med(fused_ms), min(fused_ms), max(fused_ms)),
             "  chain   time inside its five ctypes calls        median %7.3f ms per image (min %7.3f, max %7.3f)   <- the yardstick" % (med(chain_in_ms), min(chain_in_ms), max(chain_in_ms)),
             "  chain   whole wall time, NumPy glue included     median %7.3f ms per image" % med(chain_wall_ms),
             "  fused / chain (inside its calls) = %.2f" % (med(fused_ms) / med(chain_in_ms)),
             "  per image, medians:  fused  host_waits %d, bytes_up %d, bytes_down %d;   chain  host_waits %d, bytes_up %d, bytes_down %d (from its call pattern)" %
             (med(f_waits), med(f_up), med(f_down), med(c_waits), med(c_up), med(c_down)),
             "  message, state, cur_un_pts and pts_velocity equal between the two paths on every timed image: %s" % equal,
             "  the new kernels, HIP events of one more sequence of %d images:" % SEQ]
    lines += ["      %-20s %3d launches %8.2f us per launch" % (kn, n, 1e3 * ms / max(n, 1)) for kn, (n, ms) in prof.items()]
    ft.close(); backend.close()
    write(lines, OUT)
