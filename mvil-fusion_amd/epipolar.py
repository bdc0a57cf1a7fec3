"""ctypes layer over include/vilepi.h (FeatureTracker::rejectWithF and ::undistortedPoints: the camera model's lift, a RANSAC on the
fundamental matrix whose hypotheses are evaluated in parallel, the undistorted points with their velocities).

`Epipolar(cdll, camera)` drives csrc/libvilsolve.so (HIP; needs a GPU, no CPU fallback).  The only CPU restatement is
tests/epipolar_ref.py.
"""
import ctypes as C

import numpy as np

from ._row import RowError, RowHandle


class VepiCfg(C.Structure):
    _fields_ = [(k, C.c_double) for k in ("fx", "fy", "cx", "cy", "k1", "k2", "p1", "p2", "focal")] + \
               [(k, C.c_int32) for k in ("width", "height", "model", "max_points", "max_iters", "batch", "readback", "reserved")]


class VepiSummary(C.Structure):
    _fields_ = [(k, C.c_int32) for k in ("n_points", "n_inliers", "found", "best_hypothesis", "consumed", "evaluated", "launches", "reserved")]


KERNELS = ("k_epi_lift", "k_epi_hyp", "k_epi_undist")
MIN_POINTS_LIMIT, MAX_POINTS_LIMIT, MAX_ITERS_LIMIT, SAMPLE, JACOBI_SWEEPS, LIFT_STEPS = 8, 4096, 65536, 8, 10, 8
MODELS = {"PINHOLE": 0, "CATA": 1, "EQUIDISTANT": 2, "SCARAMUZZA": 3}
READBACK_PINNED, READBACK_COPY = 0, 1
DBG_CUR_PTS, DBG_FORW_PTS, DBG_SAMPLES, DBG_COUNTS, DBG_F, DBG_MARGINS = range(6)
_FP, _BP, _IP = C.POINTER(C.c_float), C.POINTER(C.c_uint8), C.POINTER(C.c_int32)
# the reference's camera (config/mynteye_leishen_indoor.yaml) and the virtual camera of rejectWithF (parameters: FOCAL_LENGTH, COL, ROW)
REFERENCE_CAMERA = dict(fx=356.37000498, fy=354.92225534, cx=326.87903275, cy=250.93806883, k1=-0.29326213, k2=0.07505211, p1=0.0002761, p2=-0.00026777,
                        focal=460.0, width=640, height=480)


class EpipolarError(RowError):
    pass


class Epipolar(RowHandle):
    ERROR, KERNELS = EpipolarError, KERNELS

    def __init__(self, cdll, camera, max_points=1024, max_iters=1000, batch=0, readback=READBACK_PINNED, model="PINHOLE", device=0):
        """camera: dict with fx, fy, cx, cy and optionally k1, k2, p1, p2, focal, width, height"""
        super().__init__(cdll, "vepi_")
        cam = dict(dict(k1=0.0, k2=0.0, p1=0.0, p2=0.0, focal=460.0, width=640, height=480), **camera)
        self.camera, self.max_points, self.max_iters = cam, max_points, max_iters
        self._n = self._evaluated = 0
        cfg = VepiCfg(*[float(cam[k]) for k in ("fx", "fy", "cx", "cy", "k1", "k2", "p1", "p2", "focal")], int(cam["width"]), int(cam["height"]), MODELS[model], max_points,
                      max_iters, batch, readback, 0)
        self._create(C.c_int32(device), C.byref(cfg))

    def reject(self, cur_xy, forw_xy, thr=1.0, confidence=0.99, seed=1, status_out=None):
        """cur_xy, forw_xy: n x 2 float32 pixels of the real camera.  Returns (status n uint8, VepiSummary)."""
        a = np.ascontiguousarray(cur_xy, np.float32).reshape(-1, 2); b = np.ascontiguousarray(forw_xy, np.float32).reshape(-1, 2)
        if len(a) != len(b):
            raise ValueError("cur_xy and forw_xy differ in length")
        n = len(a)
        st = status_out if status_out is not None else np.zeros(max(1, n), np.uint8)
        s = VepiSummary()
        self._call("reject", C.c_int32(n), a.ctypes.data_as(_FP), b.ctypes.data_as(_FP), C.c_double(thr), C.c_double(confidence), C.c_uint64(seed & (2 ** 64 - 1)),
                   st.ctypes.data_as(_BP), C.byref(s))
        if n >= SAMPLE:
            self._n, self._evaluated, self._found = n, s.evaluated, s.found
        return st[:n].copy(), s

    def undistort(self, xy, ids, dt, un_out=None, vel_out=None):
        """xy n x 2 float32 pixels, ids n int32 (-1: none), dt seconds.  Returns (un_xy, vel_xy), n x 2 float32 each."""
        p = np.ascontiguousarray(xy, np.float32).reshape(-1, 2); i = np.ascontiguousarray(ids, np.int32).reshape(-1)
        if len(p) != len(i):
            raise ValueError("xy and ids differ in length")
        n = len(p)
        un = un_out if un_out is not None else np.zeros((max(1, n), 2), np.float32)
        vel = vel_out if vel_out is not None else np.zeros((max(1, n), 2), np.float32)
        self._call("undistort", C.c_int32(n), p.ctypes.data_as(_FP), i.ctypes.data_as(_IP), C.c_double(dt), un.ctypes.data_as(_FP), vel.ctypes.data_as(_FP))
        return un[:n].copy(), vel[:n].copy()

    def reset(self):
        self._call("reset")

    def _debug(self, what, arr):
        self._call("debug_read", C.c_int32(what), C.c_void_p(arr.ctypes.data), C.c_int64(arr.nbytes))
        return arr

    def debug_points(self):
        """(p1, p2): the virtual-camera points (n x 2 float32) of the last reject() with n >= 8"""
        return self._debug(DBG_CUR_PTS, np.zeros((self._n, 2), np.float32)), self._debug(DBG_FORW_PTS, np.zeros((self._n, 2), np.float32))

    def debug_hypotheses(self):
        """(samples e x 8 int32, counts e int32, margins e float64) of the e hypotheses the last reject() evaluated"""
        e = self._evaluated
        return self._debug(DBG_SAMPLES, np.zeros((e, SAMPLE), np.int32)), self._debug(DBG_COUNTS, np.zeros(e, np.int32)), self._debug(DBG_MARGINS, np.zeros(e, np.float64))

    def debug_F(self):
        """the best hypothesis' F (3 x 3 float64) of the last reject() that found one"""
        return self._debug(DBG_F, np.zeros((3, 3), np.float64))
