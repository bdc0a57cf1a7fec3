"""The composition of include/vilfeat.h -- FeatureTracker::readImage with its bookkeeping, the updateID loop and the message -- written once,
over a pluggable backend for the arithmetic steps:
    NumpyBackend    the NumPy restatements: track_ref.RefTracker, epipolar_ref.reject / Undistorter, clahe_ref.apply;
    DeviceBackend   the device wrappers of the three rows chained through the host (track.Tracker, epipolar.Epipolar, clahe.Clahe): the
                    chain of separate calls that vfeat_read_image replaces.
Shares no code with csrc/vilfeat.hip or mvil-fusion_amd/feat.py; the device is compared with it on raw bytes."""
import numpy as np

F32, I32 = np.float32, np.int32
CHANNELS = ("points_xyz", "id", "u", "v", "vx", "vy")
COUNTS = ("n_before", "n_tracked", "n_inliers", "found", "best_hypothesis", "consumed", "n_kept", "n_candidates", "n_new", "n", "n_rows", "next_id")


class NumpyBackend:
    def __init__(self, width, height, camera, max_level, max_iters=1000, f_threshold=1.0, confidence=0.99, equalize=False, tiles=(8, 8), clip_limit=3.0):
        import epipolar_ref as er
        import track_ref as tr
        self.er, self.tr = er, tr
        self.cam = er.Camera(**dict(camera, width=width, height=height))
        self.max_level, self.max_iters, self.thr, self.confidence = max_level, max_iters, f_threshold, confidence
        self.equalize, self.tiles, self.clip_limit = equalize, tiles, clip_limit
        self.reset()

    def reset(self):
        self.t = self.tr.RefTracker(self.max_level)
        self.u = self.er.Undistorter(self.cam)

    def push(self, img):
        if self.equalize:
            import clahe_ref
            img = clahe_ref.apply(img, self.tiles[0], self.tiles[1], self.clip_limit)
        self.t.push(img)

    def track(self, pts):
        out, st = self.t.track(pts)[:2]
        return out, st

    def reject(self, cur, forw, seed):
        r = self.er.reject(self.cam, cur, forw, self.thr, self.confidence, seed, self.max_iters)
        return r.status, int(r.found), int(r.best_hypothesis), int(r.consumed)

    def detect(self, tracks, min_dist, max_cnt, quality):
        kept, new, _, _, ncand = self.t.detect(tracks, min_dist, max_cnt, quality)
        return kept, new, ncand

    def undistort(self, xy, ids, dt):
        return self.u.undistort(xy, ids, dt)

    def level(self, which, l):
        return (self.t.cur if which == "cur" else self.t.forw)[l]


class DeviceBackend:
    """the chain of today's separate calls.  calls: (name, seconds inside the ctypes call) of every row call, for tools/bench_feat.py"""

    def __init__(self, so, width, height, camera, max_level, max_points, max_candidates=1 << 16, max_iters=1000, f_threshold=1.0, confidence=0.99, equalize=False, tiles=(8, 8),
                 clip_limit=3.0):
        from mvil_fusion_amd import clahe, epipolar, track
        self.t = track.Tracker(so, width, height, max_level=max_level, max_points=max_points, max_candidates=max_candidates)
        self.e = epipolar.Epipolar(so, dict(camera, width=width, height=height), max_points=max(8, max_points), max_iters=max_iters)
        self.c = clahe.Clahe(so, width, height, tiles[0], tiles[1], clip_limit) if equalize else None
        self.thr, self.confidence = f_threshold, confidence

    def close(self):
        for r in (self.t, self.e, self.c):
            if r is not None:
                r.close()

    fresh = False

    def reset(self):
        """a first image again.  The tracker row has no call that forgets its images, so the next image goes in twice: cur = forw"""
        self.e.reset()
        self.fresh = True

    def push(self, img):
        n = 2 if self.fresh else 1
        self.fresh = False
        for _ in range(n):
            if self.c is not None:
                self.c.push(self.t, img)
            else:
                self.t.push_image(img)

    def track(self, pts):
        out, st, _ = self.t.track(pts)
        return out, st

    def reject(self, cur, forw, seed):
        st, s = self.e.reject(cur, forw, self.thr, self.confidence, seed)
        return st, int(s.found), int(s.best_hypothesis), int(s.consumed)

    def detect(self, tracks, min_dist, max_cnt, quality):
        kept, new, s = self.t.detect(tracks, min_dist, max_cnt, quality)
        return kept, new, int(s.n_candidates)

    def undistort(self, xy, ids, dt):
        return self.e.undistort(xy, ids, dt)

    def level(self, which, l):
        return self.t.debug_level(which, l)


class FeatRef:
    """readImage + updateID + message over `backend`.  After read_image: pts / ids / cnt (the state), un / vel (of all points), and
    `trace`, what the invariants of tests/test_feat_ref.py look at."""

    def __init__(self, backend, max_cnt, min_dist, quality=0.01):
        self.b, self.max_cnt, self.min_dist, self.quality = backend, max_cnt, min_dist, quality
        self.next_id = 0
        self._forget()

    def _forget(self):
        self.pts, self.ids, self.cnt = np.zeros((0, 2), F32), np.zeros(0, I32), np.zeros(0, I32)
        self.un, self.vel = np.zeros((0, 2), F32), np.zeros((0, 2), F32)
        self.prev_time = 0.0

    def reset(self):
        self._forget()
        self.b.reset()

    def read_image(self, img, time_s, publish=True, seed=0):
        b = self.b
        s = dict.fromkeys(COUNTS, 0)
        s["best_hypothesis"] = -1
        tr = dict(lost=0, rejected=0, dropped=0, priority=None)
        b.push(img)                                                                                 # step 1
        cur, ids, cnt = self.pts, self.ids, self.cnt
        forw = np.zeros((0, 2), F32)
        s["n_before"] = len(cur)
        if len(cur):                                                                                # step 2
            forw, st = b.track(cur)
            keep = st.astype(bool)
            tr["lost"] = int((~keep).sum())
            cur, forw, ids, cnt = cur[keep], forw[keep], ids[keep], cnt[keep]
        cnt = cnt + 1                                                                               # step 3
        s["n_tracked"] = s["n_inliers"] = len(forw)
        tr["after_lk"] = (ids.copy(), cnt.copy())
        if publish:
            if len(forw) >= 8:                                                                      # step 4
                st, s["found"], s["best_hypothesis"], s["consumed"] = b.reject(cur, forw, seed)
                keep = st.astype(bool)
                tr["rejected"] = int((~keep).sum())
                cur, forw, ids, cnt = cur[keep], forw[keep], ids[keep], cnt[keep]
                s["n_inliers"] = len(forw)
            order = np.argsort(-cnt.astype(np.int64), kind="stable")                                # step 5: track_cnt descending, ties in current order
            forw, ids, cnt = forw[order], ids[order], cnt[order]
            tr["priority"] = cnt.copy()
            kept, new, s["n_candidates"] = b.detect(forw, self.min_dist, self.max_cnt, self.quality)
            keep = kept.astype(bool)
            tr["dropped"] = int((~keep).sum())
            forw, ids, cnt = forw[keep], ids[keep], cnt[keep]
            s["n_kept"], s["n_new"] = len(forw), len(new)
            forw = np.concatenate([forw, np.asarray(new, F32).reshape(-1, 2)]).astype(F32)          # addPoints
            ids = np.concatenate([ids, np.full(len(new), -1, I32)]).astype(I32)
            cnt = np.concatenate([cnt, np.ones(len(new), I32)]).astype(I32)
        pts = forw                                                                                  # step 6
        tr["ids_pre"] = ids.copy()
        un, vel = b.undistort(pts, ids, time_s - self.prev_time)                                    # step 7
        un, vel = np.asarray(un, F32).reshape(-1, 2), np.asarray(vel, F32).reshape(-1, 2)
        fresh = ids == -1                                                                           # step 8
        ids = ids.copy()
        ids[fresh] = self.next_id + np.arange(int(fresh.sum()), dtype=I32)
        self.next_id += int(fresh.sum())
        self.pts, self.ids, self.cnt, self.un, self.vel, self.prev_time = pts, ids, cnt, un, vel, time_s
        rows = cnt > 1 if publish else np.zeros(len(cnt), bool)                                     # step 9
        msg = dict(points_xyz=np.concatenate([un[rows], np.ones((int(rows.sum()), 1), F32)], axis=1).astype(F32), id=ids[rows].astype(F32), u=pts[rows, 0].copy(),
                   v=pts[rows, 1].copy(), vx=vel[rows, 0].copy(), vy=vel[rows, 1].copy())
        s["n"], s["n_rows"], s["next_id"] = len(pts), int(rows.sum()), self.next_id
        self.trace = tr
        return msg, s


# ---- the test scene of the issue: a drifting texture with an independently moving block -----------------------------------------------------
def camera(width, height):
    return dict(fx=0.72 * width, fy=0.72 * width, cx=width / 2 - 3, cy=height / 2 + 2, k1=-0.28, k2=0.07, p1=2e-4, p2=-1e-4, focal=460.0)


def scene_image(height, width, k):
    from mvil_fusion_amd import track
    img = track.Texture(height, width, seed=7).render((1.3 * k + 0.4 * np.sin(0.9 * k), -0.7 * k)).copy()
    blk = track.Texture(height, width, seed=21).render((-2.1 * k, 1.6 * k))
    x0, y0 = int(width // 2 - 14 - np.rint(2.1 * k)), int(height // 2 - 14 + np.rint(1.6 * k))
    img[y0:y0 + 28, x0:x0 + 28] = blk[y0:y0 + 28, x0:x0 + 28]
    return img


SMALL = dict(height=96, width=128, max_level=1, min_dist=10, max_cnt=40, max_iters=64)
LARGE = dict(height=192, width=256, max_level=3, min_dist=6, max_cnt=300, max_iters=128)


def time_of(k):
    return 0.1 * k


def seed_of(k):
    return 1000 + k
