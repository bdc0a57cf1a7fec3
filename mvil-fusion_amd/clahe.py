"""ctypes layer over include/vilclahe.h (CLAHE, the first step of FeatureTracker::readImage under `equalize: 1`): a raw 8-bit image in,
the equalised image out or, fused, straight into the resident tracker's next image (mvil-fusion_amd/track.py).

`Clahe(cdll, width, height)` drives csrc/libvilsolve.so (HIP; needs a GPU, no CPU fallback).  The only CPU restatement is
tests/clahe_ref.py.
"""
import ctypes as C

import numpy as np

from ._row import RowError, RowHandle


class VclaheCfg(C.Structure):
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("tiles_x", C.c_int32), ("tiles_y", C.c_int32), ("clip_limit", C.c_double)]


KERNELS = ("k_clahe_hist", "k_clahe_lut", "k_clahe_blend")
MAX_TILES = 16
DBG_HIST, DBG_LUT = range(2)


class ClaheError(RowError):
    pass


class Clahe(RowHandle):
    ERROR, KERNELS = ClaheError, KERNELS

    def __init__(self, cdll, width, height, tiles_x=8, tiles_y=8, clip_limit=3.0, device=0):
        super().__init__(cdll, "vclahe_")
        self.width, self.height, self.tiles_x, self.tiles_y, self.clip_limit = width, height, tiles_x, tiles_y, clip_limit
        cfg = VclaheCfg(width, height, tiles_x, tiles_y, clip_limit)
        self._create(C.c_int32(device), C.byref(cfg))

    def _image(self, gray, row_stride):
        g = np.asarray(gray, np.uint8)
        if row_stride is None:
            g = np.ascontiguousarray(g); row_stride = g.shape[1] if g.ndim == 2 else self.width
        return g, row_stride

    def apply(self, gray, row_stride=None, out=None):
        """gray: height x width uint8 (any row stride >= width in bytes).  Returns the equalised image; out: the array to write into."""
        g, row_stride = self._image(gray, row_stride)
        out = out if out is not None else np.zeros((self.height, self.width), np.uint8)
        self._call("apply", C.c_void_p(g.ctypes.data), C.c_int32(row_stride), C.c_void_p(out.ctypes.data), C.c_int32(out.strides[0]))
        return out

    def push(self, tracker, gray, want_equalised=False, row_stride=None):
        """Equalise gray into `tracker` (a track.Tracker of the same size): what tracker.push_image(apply(gray)) does, in one submission
        and without the round trip.  Returns the equalised image when want_equalised, else None."""
        g, row_stride = self._image(gray, row_stride)
        out = np.zeros((self.height, self.width), np.uint8) if want_equalised else None
        self._call("push", tracker.ctx, C.c_void_p(g.ctypes.data), C.c_int32(row_stride), C.c_void_p(out.ctypes.data if want_equalised else None),
                   C.c_int32(self.width if want_equalised else 0))
        return out

    def _debug(self, what, arr):
        self._call("debug_read", C.c_int32(what), C.c_void_p(arr.ctypes.data), C.c_int64(arr.nbytes))
        return arr

    def debug_hist(self):
        """the tiles' histograms after clipping and redistribution, [tiles_y][tiles_x][256] int32, of the last apply() / push()"""
        return self._debug(DBG_HIST, np.zeros((self.tiles_y, self.tiles_x, 256), np.int32))

    def debug_lut(self):
        """the tiles' LUTs, [tiles_y][tiles_x][256] uint8, of the last apply() / push()"""
        return self._debug(DBG_LUT, np.zeros((self.tiles_y, self.tiles_x, 256), np.uint8))
