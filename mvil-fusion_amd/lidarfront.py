"""ctypes layer over include/vilfront.h: Estimator::processLidar from the de-skew to the alignment and its fitness as one resident call.

`LidarFront(cdll)` drives csrc/libvilsolve.so (HIP; needs a GPU, no CPU fallback).  The only CPU restatement of the de-skew is
tests/lidarfront_ref.py; everything behind it is the cloud, vgicp and loopverify rows.
"""
import ctypes as C

import numpy as np

from ._row import RowError, RowHandle
from .vgicp import VgicpOptions, VgicpSummary


class VfrontMotion(C.Structure):
    _fields_ = [("q", C.c_float * 4), ("t", C.c_float * 3), ("reserved", C.c_float)]


class VfrontOptions(C.Structure):
    _fields_ = [("deskew", C.c_int32), ("hist_size", C.c_int32), ("lidar_time_step", C.c_double), ("min_distance", C.c_double), ("max_distance", C.c_double),
                ("resolution", C.c_double), ("leaf", C.c_float), ("reserved", C.c_int32), ("reg", VgicpOptions)]


class VfrontSummary(C.Structure):
    _fields_ = [("n_raw", C.c_int32), ("n_kept", C.c_int32), ("n_filtered", C.c_int32), ("accepted", C.c_int32), ("aligned", C.c_int32), ("n_used", C.c_int32),
                ("fitness", C.c_double), ("T", C.c_double * 16), ("reg", VgicpSummary)]


KERNELS = ("k_front_deskew", "k_front_scan", "k_front_scatter", "k_front_xyz")
KNN = 20
DBG_DESKEWED, DBG_FILTERED = 0, 1
ERR_INVALID_ARGUMENT, ERR_DEVICE, ERR_NON_FINITE = -1, -2, -3
_FP = C.POINTER(C.c_float)
_DP = C.POINTER(C.c_double)


class LidarFrontError(RowError):
    pass


def default_options(cdll, **kw):
    """vfront_default_options; keyword arguments set fields of vfront_options, or of its vgicp_options when they are not its own."""
    o = VfrontOptions()
    f = cdll.vfront_default_options; f.restype = None
    f(C.byref(o))
    for k, v in kw.items():
        if k in dict(VfrontOptions._fields_) and k != "reg":
            setattr(o, k, v)
        elif k in dict(VgicpOptions._fields_):
            setattr(o.reg, k, v)
        else:
            raise AttributeError("vfront_options has no field %r" % k)
    return o


def motion(q_wxyz, t):
    """A vfront_motion from the float quaternion (w, x, y, z) and the float translation of TransformToEnd."""
    m = VfrontMotion()
    m.q[:] = [float(v) for v in np.asarray(q_wxyz, np.float32).reshape(4)]
    m.t[:] = [float(v) for v in np.asarray(t, np.float32).reshape(3)]
    return m


def summary_bytes(s):
    """The raw bytes of a VfrontSummary (or of any ctypes structure): what the byte-for-byte tests compare."""
    return bytes(memoryview(s).cast("B"))


class LidarFront(RowHandle):
    ERROR, KERNELS = LidarFrontError, KERNELS

    def __init__(self, cdll, max_scan_points=1 << 15, device=0):
        super().__init__(cdll, "vfront_")
        self.max_scan_points = max_scan_points
        self._create(C.c_int32(device), C.c_int32(max_scan_points))

    def reset(self):
        self._call("reset")

    def set_grid(self, min_points, cell):
        self._call("set_grid", C.c_int32(min_points), C.c_double(cell))

    def push_scan(self, xyzi, mot=None, guess=None, opts=None):
        """One scan: n x 4 float32 raw points, a VfrontMotion (None only with deskew = 0), a 4 x 4 float64 guess or None (the identity),
        VfrontOptions or None (the defaults).  Returns the VfrontSummary."""
        xyzi = np.ascontiguousarray(xyzi, np.float32).reshape(-1, 4)
        g = None if guess is None else np.ascontiguousarray(guess, np.float64).reshape(16)
        s = VfrontSummary()
        self._call("push_scan", C.c_int32(len(xyzi)), xyzi.ctypes.data_as(_FP), C.byref(mot) if mot is not None else None,
                   g.ctypes.data_as(_DP) if g is not None else None, C.byref(opts) if opts is not None else None, C.byref(s))
        return s

    def _read(self, name, *args):
        n = C.c_int32(0)
        st = self._f(name)(self.ctx, *args, None, C.c_int32(0), C.byref(n))                     # capacity 0: the status is "invalid" unless there is nothing, n is set
        if n.value == 0:
            self._chk(name, st)
        out = np.zeros((max(1, n.value), 4), np.float32)
        self._call(name, *args, out.ctypes.data_as(_FP), C.c_int32(n.value), C.byref(n))
        return out[:n.value]

    def read_deskewed(self):
        """The de-skewed cloud with its removed points gone, n_kept x 4 float32."""
        return self._read("read_deskewed")

    def debug_read(self, stage):
        """DBG_DESKEWED or DBG_FILTERED of the last scan that reached the device."""
        return self._read("debug_read", C.c_int32(stage))
