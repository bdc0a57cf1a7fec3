"""ctypes layer over include/vilfeat.h (FeatureTracker::readImage as one call: camera image in, the feature message out, the points, ids,
track counts and the velocity table resident on the device in between).

`FeatureTracker(cdll, width, height, camera)` drives csrc/libvilsolve.so (HIP; needs a GPU, no CPU fallback).  The only CPU restatement
of the composition is tests/feat_ref.py.
"""
import ctypes as C

import numpy as np

from ._row import RowError, RowHandle
from .epipolar import MODELS

_FP = C.POINTER(C.c_float)


class VfeatCfg(C.Structure):
    _fields_ = [(k, C.c_double) for k in ("fx", "fy", "cx", "cy", "k1", "k2", "p1", "p2", "focal", "clip_limit", "f_threshold", "confidence")] + [("quality", C.c_float)] + \
               [(k, C.c_int32) for k in ("width", "height", "max_level", "max_points", "max_candidates", "model", "max_iters", "equalize", "tiles_x", "tiles_y", "max_cnt",
                                         "min_dist", "reserved")]


class VfeatMsg(C.Structure):
    _fields_ = [(k, _FP) for k in ("points_xyz", "id", "u", "v", "vx", "vy")] + [("n_rows", C.c_int32), ("reserved", C.c_int32)]


class VfeatSummary(C.Structure):
    _fields_ = [(k, C.c_int32) for k in ("n_before", "n_tracked", "n_inliers", "found", "best_hypothesis", "consumed", "n_records", "n_kept", "n_candidates", "n_new", "n",
                                         "n_rows", "next_id", "host_waits")] + [("bytes_up", C.c_int64), ("bytes_down", C.c_int64)]


KERNELS = ("k_feat_compact_lk", "k_feat_records", "k_feat_compact_rank", "k_feat_compact_add", "k_feat_finish")
MIN_POINTS_LIMIT, MAX_POINTS_LIMIT, HEADER_BYTES, ROW_BYTES = 8, 4096, 64, 32
DBG_STATE, DBG_UN_VEL, DBG_CUR_LEVEL, DBG_FORW_LEVEL = range(4)
CHANNELS = ("points_xyz", "id", "u", "v", "vx", "vy")


class FeatError(RowError):
    pass


class FeatureTracker(RowHandle):
    ERROR, KERNELS = FeatError, KERNELS

    def __init__(self, cdll, width, height, camera, max_level=3, max_points=None, max_candidates=1 << 16, max_iters=1000, equalize=False, tiles_x=8, tiles_y=8, clip_limit=3.0,
                 max_cnt=150, min_dist=30, quality=0.01, f_threshold=1.0, confidence=0.99, model="PINHOLE", device=0):
        """camera: dict with fx, fy, cx, cy and optionally k1, k2, p1, p2, focal"""
        super().__init__(cdll, "vfeat_")
        cam = dict(dict(k1=0.0, k2=0.0, p1=0.0, p2=0.0, focal=460.0), **camera)
        self.width, self.height, self.max_level, self.max_cnt = width, height, max_level, max_cnt
        self.max_points = max(MIN_POINTS_LIMIT, max_cnt) if max_points is None else max_points
        self.images = 0
        cfg = VfeatCfg(*[float(cam[k]) for k in ("fx", "fy", "cx", "cy", "k1", "k2", "p1", "p2", "focal")], float(clip_limit), float(f_threshold), float(confidence),
                       float(quality), width, height, max_level, self.max_points, max_candidates, MODELS[model], max_iters, int(equalize), tiles_x, tiles_y, max_cnt, min_dist, 0)
        self._create(C.c_int32(device), C.byref(cfg))

    def new_message(self):
        """the caller-owned arrays of a message: dict of float32 arrays with room for max_cnt rows"""
        m = max(1, self.max_cnt)
        return {k: np.zeros((m, 3) if k == "points_xyz" else m, np.float32) for k in CHANNELS}

    def read_image(self, gray, time_s, publish=True, seed=None, row_stride=None, into=None):
        """gray: height x width uint8.  seed=None: the image counter.  Returns (message, VfeatSummary): message is a dict of the arrays cut
        to n_rows (copies), {} with rows 0 when not published.  into: the arrays to write into (tests of the error paths)."""
        g = np.asarray(gray, np.uint8)
        if row_stride is None:
            g = np.ascontiguousarray(g); row_stride = g.shape[1] if g.ndim == 2 else self.width
        arrays = into if into is not None else self.new_message()
        msg = VfeatMsg(*[arrays[k].ctypes.data_as(_FP) for k in CHANNELS], -1, 0)
        s = VfeatSummary()
        seed = self.images if seed is None else seed
        self._call("read_image", C.c_void_p(g.ctypes.data), C.c_int32(row_stride), C.c_double(time_s), C.c_int32(1 if publish else 0), C.c_uint64(seed & (2 ** 64 - 1)),
                   C.byref(msg), C.byref(s))
        self.images += 1
        return {k: arrays[k][:msg.n_rows].copy() for k in CHANNELS}, s

    def reset(self):
        self._call("reset")

    def _debug(self, what, arg, arr):
        self._call("debug_read", C.c_int32(what), C.c_int32(arg), C.c_void_p(arr.ctypes.data), C.c_int64(arr.nbytes))
        return arr

    def debug_state(self):
        """(cur_pts n x 2 float32, ids n int32 after updateID, track_cnt n int32)"""
        raw = self._debug(DBG_STATE, 0, np.zeros(4 + 16 * self.max_points, np.uint8))
        n = int(raw[:4].view(np.int32)[0])
        return (raw[4:4 + 8 * n].view(np.float32).reshape(n, 2).copy(), raw[4 + 8 * n:4 + 12 * n].view(np.int32).copy(), raw[4 + 12 * n:4 + 16 * n].view(np.int32).copy())

    def debug_un_vel(self):
        """(cur_un_pts, pts_velocity), n x 2 float32 each, of all points -- also after an unpublished image"""
        n = len(self.debug_state()[1])
        raw = self._debug(DBG_UN_VEL, 0, np.zeros((2, max(1, n), 2), np.float32)) if n else np.zeros((2, 0, 2), np.float32)
        return raw[0].copy(), raw[1].copy()

    def level_shape(self, level):
        h, w = self.height, self.width
        for _ in range(level):
            h, w = (h + 1) // 2, (w + 1) // 2
        return h, w

    def debug_level(self, which, level):
        """a pyramid level (uint8) of "cur" or "forw" of the owned tracker"""
        return self._debug(DBG_CUR_LEVEL if which == "cur" else DBG_FORW_LEVEL, level, np.zeros(self.level_shape(level), np.uint8))
