"""ctypes layer over include/viltrack.h (the KLT visual front end of FeatureTracker::readImage: pyramidal LK tracking, setMask and
min-eigenvalue corner detection) + the synthetic texture and image sequence the tests and tools/bench_track.py share.

`Tracker(cdll, width, height)` drives csrc/libvilsolve.so (HIP; needs a GPU, no CPU fallback).  The only CPU restatement is
tests/track_ref.py.
"""
import ctypes as C

import numpy as np

from ._row import RowError, RowHandle


class VtrackCfg(C.Structure):
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("max_level", C.c_int32), ("max_points", C.c_int32), ("max_candidates", C.c_int32)]


class VtrackSummary(C.Structure):
    _fields_ = [("n_points", C.c_int32), ("n_tracked", C.c_int32), ("n_tracks", C.c_int32), ("n_kept", C.c_int32), ("n_candidates", C.c_int32), ("n_picked", C.c_int32),
                ("n_new", C.c_int32), ("rounds", C.c_int32)]


KERNELS = ("k_track_pyr", "k_track_lk", "k_track_mask", "k_track_paint", "k_track_eig", "k_track_cand", "k_track_round", "k_track_pick")
MAX_LEVEL, MAX_POINTS_LIMIT, MAX_MIN_DIST = 3, 4096, 1024
CODES = {"SKIP": 0, "LOWEIG": 1, "EPS": 2, "OSC": 3, "CAP": 4, "OOB": 5}
DBG_CUR_LEVEL, DBG_FORW_LEVEL, DBG_LK_CODES, DBG_LK_ITERS, DBG_EIG, DBG_MASK, DBG_N_CANDIDATES = range(7)
_FP, _BP = C.POINTER(C.c_float), C.POINTER(C.c_uint8)


class TrackError(RowError):
    pass


class Tracker(RowHandle):
    ERROR, KERNELS = TrackError, KERNELS

    def __init__(self, cdll, width, height, max_level=3, max_points=1024, max_candidates=1 << 16, device=0):
        super().__init__(cdll, "vtrack_")
        self.width, self.height, self.max_level, self.max_points, self.max_candidates = width, height, max_level, max_points, max_candidates
        self._n = 0
        cfg = VtrackCfg(width, height, max_level, max_points, max_candidates)
        self._create(C.c_int32(device), C.byref(cfg))

    def level_shape(self, level):
        h, w = self.height, self.width
        for _ in range(level):
            h, w = (h + 1) // 2, (w + 1) // 2
        return h, w

    def push_image(self, gray, row_stride=None):
        """gray: height x width uint8 (any row stride >= width in bytes).  It becomes forw, the last forw becomes cur."""
        g = np.asarray(gray, np.uint8)
        if row_stride is None:
            g = np.ascontiguousarray(g); row_stride = g.shape[1] if g.ndim == 2 else self.width
        self._keep = g
        self._call("push_image", C.c_void_p(g.ctypes.data), C.c_int32(row_stride))

    def track(self, cur_xy, forw_out=None, status_out=None):
        """cur_xy n x 2 float32 pixel positions in cur.  Returns (forw_xy n x 2 float32, status n uint8, VtrackSummary).  forw_out /
        status_out: arrays to write into (tests of the error path)."""
        pts = np.ascontiguousarray(cur_xy, np.float32).reshape(-1, 2)
        n = len(pts)
        forw = forw_out if forw_out is not None else np.zeros((max(1, n), 2), np.float32)
        st = status_out if status_out is not None else np.zeros(max(1, n), np.uint8)
        s = VtrackSummary()
        self._call("track", C.c_int32(n), pts.ctypes.data_as(_FP), forw.ctypes.data_as(_FP), st.ctypes.data_as(_BP), C.byref(s))
        self._n = n
        return forw[:n].copy(), st[:n].copy(), s

    def detect(self, tracks_xy, min_dist, max_cnt, quality=0.01, kept_out=None, new_out=None):
        """tracks_xy n x 2 float32 in priority order.  Returns (kept n uint8, new_xy m x 2 float32 in pick order, VtrackSummary)."""
        tr = np.ascontiguousarray(tracks_xy, np.float32).reshape(-1, 2)
        n = len(tr)
        kept = kept_out if kept_out is not None else np.zeros(max(1, n), np.uint8)
        new = new_out if new_out is not None else np.zeros((max(1, max_cnt), 2), np.float32)
        n_new = C.c_int32(-1)
        s = VtrackSummary()
        self._call("detect", C.c_int32(n), tr.ctypes.data_as(_FP), C.c_int32(min_dist), C.c_int32(max_cnt), C.c_float(quality), kept.ctypes.data_as(_BP), C.byref(n_new),
                   new.ctypes.data_as(_FP), C.byref(s))
        return kept[:n].copy(), new[:n_new.value].copy(), s

    def _debug(self, what, arg, arr):
        self._call("debug_read", C.c_int32(what), C.c_int32(arg), C.c_void_p(arr.ctypes.data), C.c_int64(arr.nbytes))
        return arr

    def debug_level(self, which, level):
        """a pyramid level (uint8) of "cur" or "forw" """
        return self._debug(DBG_CUR_LEVEL if which == "cur" else DBG_FORW_LEVEL, level, np.zeros(self.level_shape(level), np.uint8))

    def debug_lk(self):
        """(codes, iters), each n x (max_level + 1) uint8 with column l = level l, of the last track()"""
        shape = (max(1, self._n), self.max_level + 1)
        c = self._debug(DBG_LK_CODES, 0, np.zeros(shape, np.uint8)); i = self._debug(DBG_LK_ITERS, 0, np.zeros(shape, np.uint8))
        return c[:self._n], i[:self._n]

    def debug_detect(self):
        """(eig float32 map, mask uint8 map, candidate count) of the last detect()"""
        hw = (self.height, self.width)
        return self._debug(DBG_EIG, 0, np.zeros(hw, np.float32)), self._debug(DBG_MASK, 0, np.zeros(hw, np.uint8)), int(self._debug(DBG_N_CANDIDATES, 0, np.zeros(1, np.int32))[0])


# ---- synthetic texture: a sum of seeded sinusoids, so that a shifted image is the same function evaluated elsewhere ------------------
class Texture:
    """f(x, y) = sum_k a_k sin(u_k x + v_k y + phi_k), 40 terms with |u|, |v| <= 0.35 rad/px, scaled so that the unshifted height x width
    image spans 128 +- 100.  render(shift) is the image of the texture moved BY shift = (sx, sy): a feature at p appears at p + shift."""

    def __init__(self, height, width, seed=0, terms=40, max_freq=0.35):
        rng = np.random.default_rng(seed)
        self.height, self.width = height, width
        self.u = rng.uniform(-max_freq, max_freq, terms); self.v = rng.uniform(-max_freq, max_freq, terms)
        self.phi = rng.uniform(0, 2 * np.pi, terms); self.a = rng.uniform(0.5, 1.0, terms)
        self.scale = 100.0 / np.abs(self._f(0.0, 0.0)).max()

    def _f(self, sx, sy):
        y, x = np.mgrid[0:self.height, 0:self.width].astype(np.float64)
        x = x - sx; y = y - sy
        out = np.zeros_like(x)
        for u, v, p, a in zip(self.u, self.v, self.phi, self.a):
            out += a * np.sin(u * x + v * y + p)
        return out

    def render(self, shift=(0.0, 0.0), noise=0.0, seed=0):
        img = 128.0 + self.scale * self._f(float(shift[0]), float(shift[1]))
        if noise:
            img = img + np.random.default_rng(seed).normal(0.0, noise, img.shape)
        return np.clip(np.rint(img), 0, 255).astype(np.uint8)


def interior_points(height, width, n, margin, seed=0):
    """n float32 points at least `margin` px inside the image"""
    rng = np.random.default_rng(seed)
    return np.stack([rng.uniform(margin, width - 1 - margin, n), rng.uniform(margin, height - 1 - margin, n)], axis=1).astype(np.float32)


def sequence(height, width, n_images, seed=0, step=(1.3, -0.7), noise=0.0):
    """(images, shifts): image k is the texture moved by shifts[k]; the shift drifts by about `step` px per image with a slow wobble"""
    tex = Texture(height, width, seed)
    shifts = [(k * step[0] + 0.4 * np.sin(0.9 * k), k * step[1] + 0.3 * np.cos(0.7 * k) - 0.3) for k in range(n_images)]
    return [tex.render(s, noise=noise, seed=seed + k) for k, s in enumerate(shifts)], shifts
