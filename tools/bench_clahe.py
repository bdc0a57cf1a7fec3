"""Wall time and per-kernel HIP-event time of CLAHE in front of the KLT front end (include/vilclahe.h).
  workload  640 x 480, tiles 8 x 8, clip limit 3.0 (the reference's), the synthetic sequence of mvil-fusion_amd/track.py with noise sigma 2;
            the tracker at max_level 3.  Three entry points on the same images in the same run:
              vclahe_apply       raw image up, equalised image back;
              vclahe_push        raw image up, equalised into the tracker's next image, pyramid built -- with and without reading the
                                 equalised image back;
              vtrack_push_image  the yardstick: an (already equalised) image up, pyramid built, on the same tracker.
Wall = host clock around the call, median of 5 calls after a warm-up of 3, events off; kernels = HIP events of 5 more calls.
There is no compiled CPU opponent on these machines (no OpenCV), so nothing here is a speed-up; the NumPy restatement's time
(tests/clahe_ref.py) is given as what it is.  Written to profiles/clahe.txt (OUT=<file> for another place).

    python tools/bench_clahe.py [calls, default 5]"""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import __graft_entry__ as g; g.load_package()
from mvil_fusion_amd import clahe, lib, track
from _rowbench import device_name, write
from bench_posegraph import host_name, source_state

OUT = os.environ.get("OUT") or os.path.join(ROOT, "profiles", "clahe.txt")
W, H, TILES, CLIP, LEVELS, WARM = 640, 480, 8, 3.0, 3, 3


def measure(name, fn, rows, images, calls):
    """fn(image) timed on `calls` images after WARM, then `calls` more with the events of `rows` on: (median wall ms, lines)"""
    for k in range(WARM):
        fn(images[k])
    ts = []
    for k in range(calls):
        a = time.perf_counter(); fn(images[WARM + k]); ts.append(time.perf_counter() - a)
    ts = 1e3 * np.array(ts)
    for r in rows:
        r.profile_enable(True); r.profile_read()
    for k in range(calls):
        fn(images[WARM + calls + k])
    prof = {}
    for r in rows:
        prof.update({kn: v for kn, v in r.profile_read().items() if v[0]})
        r.profile_enable(False)
    kt = sum(ms for _, ms in prof.values()) / calls
    lines = ["  %-34s wall median %7.3f ms, min %7.3f, max %7.3f; kernels %7.3f ms per call; the rest %7.3f ms (copies, launches, the synchronisation)" %
             (name, np.median(ts), ts.min(), ts.max(), kt, np.median(ts) - kt)]
    lines += ["      %-14s %3d launches %8.3f ms per call" % (kn, n, ms / calls) for kn, (n, ms) in prof.items()]
    return float(np.median(ts)), lines


if __name__ == "__main__":
    calls = max(2, int(sys.argv[1])) if len(sys.argv) > 1 else 5
    so = lib.load_vilsolve()
    images, _ = track.sequence(H, W, WARM + 2 * calls, seed=1, noise=2.0)
    t = track.Tracker(so, W, H, max_level=LEVELS, max_points=150, max_candidates=1 << 16)
    c = clahe.Clahe(so, W, H, TILES, TILES, CLIP)
    equalised = [c.apply(img) for img in images]
    lines = ["CLAHE in front of the KLT front end (include/vilclahe.h); %s; host %s; %s" % (device_name(), host_name(), source_state()),
             "%d x %d, tiles %d x %d, clip limit %g, tracker max_level %d; wall = host clock around the call, medians of %d calls after %d, events off;" %
             (W, H, TILES, TILES, CLIP, LEVELS, calls, WARM),
             "kernels = HIP events of %d more calls.  No compiled CPU opponent exists on these machines (no OpenCV): this is not a speed-up table." % calls]
    out = np.zeros((H, W), np.uint8)
    _, l = measure("vclahe_apply", lambda img: c.apply(img, out=out), (c,), images, calls); lines += l
    push, l = measure("vclahe_push", lambda img: c.push(t, img), (c, t), images, calls); lines += l
    _, l = measure("vclahe_push, equalised read back", lambda img: c.push(t, img, want_equalised=True), (c, t), images, calls); lines += l
    yard, l = measure("vtrack_push_image (yardstick)", t.push_image, (t,), equalised, calls); lines += l
    lines.append("  vclahe_push / vtrack_push_image = %.2f by wall time: what equalising on the device adds to an image's push" % (push / yard))
    import clahe_ref
    a = time.perf_counter(); ref = clahe_ref.apply(images[0], TILES, TILES, CLIP); b = time.perf_counter()
    lines.append("  the NumPy restatement (tests/clahe_ref.py, one call, this host): %.0f ms; the device's image equals it: %s" % (1e3 * (b - a), bool((ref == equalised[0]).all())))
    t.close(); c.close()
    write(lines, OUT)
