"""Wall time and per-kernel HIP-event time of the KLT front end (include/viltrack.h) per camera image.
  workload  640 x 480, max_level 3, min_dist 30, quality 0.01, the synthetic sequence of mvil-fusion_amd/track.py (a sum of sinusoids that
            drifts by about (1.3, -0.7) px per image, noise sigma 2).  Per image, as readImage does it: vtrack_push_image, vtrack_track of N
            points, compaction on the status, vtrack_detect with max_cnt = N, the new corners appended.  At min_dist 30 the image holds
            about 250 corners, so the tracked set is topped up to N with random interior points before every vtrack_track.
  N         150 (the reference's MAX_CNT), 64 and 1000.
Wall = host clock around each entry point, medians of 5 images after a warm-up of 3, events off; kernels = HIP events of 5 more images.
There is no compiled CPU opponent on these machines (no OpenCV), so nothing here is a speed-up.  Written to profiles/track.txt
(OUT=<file> for another place).

    python tools/bench_track.py [images, default 5]

Every N runs in a child process of its own under a time limit of its own; one that fails or runs out of time ends the run, what was measured
until then is still written."""
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import __graft_entry__ as g; g.load_package()
from mvil_fusion_amd import lib, track
from _rowbench import device_name, write
from bench_posegraph import host_name, source_state

OUT = os.environ.get("OUT") or os.path.join(ROOT, "profiles", "track.txt")
W, H, LEVELS, MIN_DIST, QUALITY, WARM = 640, 480, 3, 30, 0.01, 3
POINTS = (150, 64, 1000)
PUSH, TRACK, DETECT = ("k_track_pyr",), ("k_track_lk",), ("k_track_mask", "k_track_paint", "k_track_eig", "k_track_cand", "k_track_round", "k_track_pick")


def med(ts):
    ts = 1e3 * np.array(ts)
    return "median %7.3f ms, min %7.3f, max %7.3f" % (np.median(ts), ts.min(), ts.max())


def one(n, images_timed):
    so = lib.load_vilsolve()
    n_img = WARM + 2 * images_timed
    images, _ = track.sequence(H, W, n_img, seed=1, noise=2.0)
    t = track.Tracker(so, W, H, max_level=LEVELS, max_points=n, max_candidates=1 << 16)
    pts = np.zeros((0, 2), np.float32)
    wall = {"push_image": [], "track": [], "detect": [], "image": []}
    stats = {"tracked": [], "kept": [], "cand": [], "new": [], "rounds": [], "depth_max": [], "depth_mean": []}
    prof = {"push_image": {}, "track": {}, "detect": {}}
    for k, img in enumerate(images):
        timed, events = WARM <= k < WARM + images_timed, k >= WARM + images_timed
        if k == WARM + images_timed:
            t.profile_enable(True); t.profile_read()
        fill = track.interior_points(H, W, n - len(pts), 24, seed=100 + k) if len(pts) < n else np.zeros((0, 2), np.float32)
        cur = np.concatenate([pts, fill])[:n]
        a = time.perf_counter(); t.push_image(img); b = time.perf_counter()
        out, st, s1 = t.track(cur); c = time.perf_counter()
        alive = out[st == 1]
        d0 = time.perf_counter(); kept, new, s2 = t.detect(alive, MIN_DIST, n, QUALITY); d = time.perf_counter()
        pts = np.concatenate([alive[kept == 1], new])[:n]
        if timed:
            wall["push_image"].append(b - a); wall["track"].append(c - b); wall["detect"].append(d - d0); wall["image"].append((b - a) + (c - b) + (d - d0))
        if events:
            p = t.profile_read()
            for name, ks in (("push_image", PUSH), ("track", TRACK), ("detect", DETECT)):
                for kn in ks:
                    l0, m0 = prof[name].get(kn, (0, 0.0)); prof[name][kn] = (l0 + p[kn][0], m0 + p[kn][1])
            codes, iters = t.debug_lk()
            depth = iters.astype(np.int64).sum(axis=1)
            stats["depth_max"].append(depth.max()); stats["depth_mean"].append(depth.mean())
            stats["tracked"].append(s1.n_tracked); stats["kept"].append(s2.n_kept); stats["cand"].append(s2.n_candidates); stats["new"].append(s2.n_new); stats["rounds"].append(s2.rounds)
    t.close()
    m = {k: float(np.mean(v)) for k, v in stats.items()}
    lines = ["%d points: %.0f tracked, %.0f kept by setMask, %.0f candidates, %.0f new corners, %.1f fixpoint rounds per image (means of %d images)" %
             (n, m["tracked"], m["kept"], m["cand"], m["new"], m["rounds"], images_timed),
             "  LK iterations summed over the 4 levels: mean %.1f per point, the slowest point of an image %.0f (cap 120): the launch's serial depth" % (m["depth_mean"], m["depth_max"])]
    ksum = 0.0
    for name in ("push_image", "track", "detect"):
        kt = sum(ms for _, ms in prof[name].values()) / images_timed
        ksum += kt
        lines.append("  %-11s wall %s; kernels %7.3f ms per image; the rest %7.3f ms (copies, launches, the synchronisation)" %
                     (name, med(wall[name]), kt, 1e3 * np.median(wall[name]) - kt))
        lines += ["      %-14s %3d launches %8.3f ms per image" % (kn, ln, ms / images_timed) for kn, (ln, ms) in prof[name].items()]
    lines.append("  per image   wall %s; kernels %7.3f ms" % (med(wall["image"]), ksum))
    return lines


if __name__ == "__main__":
    if len(sys.argv) > 3 and sys.argv[1] == "--one":
        print("\n".join(one(int(sys.argv[2]), int(sys.argv[3]))))
        sys.exit(0)
    images_timed = max(2, int(sys.argv[1])) if len(sys.argv) > 1 else 5
    lines = ["KLT front end (include/viltrack.h); %s; host %s; %s" % (device_name(), host_name(), source_state()),
             "%d x %d, max_level %d, min_dist %d, quality %g; wall = host clock around each entry point, medians of %d images after %d, events off;" % (W, H, LEVELS, MIN_DIST, QUALITY, images_timed, WARM),
             "kernels = HIP events of %d more images.  No compiled CPU opponent exists on these machines (no OpenCV): this is not a speed-up table." % images_timed]
    for n in POINTS:
        print("running", n, file=sys.stderr, flush=True)
        args = ["--one", str(n), str(images_timed)]
        try:
            p = subprocess.run([sys.executable, os.path.abspath(__file__)] + args, capture_output=True, text=True, timeout=120)
        except subprocess.TimeoutExpired:
            lines.append("%s: no result within 120 s; the run ends here" % " ".join(args))
            write(lines, OUT); sys.exit(1)
        if p.returncode != 0:
            lines.append("%s: exit status %d; the run ends here\n%s" % (" ".join(args), p.returncode, p.stderr[-1000:]))
            write(lines, OUT); sys.exit(1)
        lines.append(p.stdout.rstrip("\n"))
    write(lines, OUT)
