"""ctypes layer over include/vilcloud.h: the feature tracker's accumulated depth cloud, resident on the device (lidar_callback), and
pcl::ApproximateVoxelGrid as a stand-alone call.

`DepthCloud(cdll)` drives csrc/libvilsolve.so (HIP; needs a GPU, no CPU fallback).  The only CPU restatement is tests/cloud_ref.py.
"""
import ctypes as C

import numpy as np

from ._row import RowError, RowHandle


class VcloudOptions(C.Structure):
    _fields_ = [("leaf_scan", C.c_float), ("leaf_cloud", C.c_float), ("hist_size", C.c_int32), ("max_coord", C.c_float), ("max_ratio", C.c_float),
                ("reserved", C.c_int32), ("window_s", C.c_double)]


class VcloudSummary(C.Structure):
    _fields_ = [("n_raw", C.c_int32), ("n_scan_ds", C.c_int32), ("n_in_view", C.c_int32), ("n_scans", C.c_int32), ("n_popped", C.c_int32),
                ("n_fused", C.c_int32), ("n_cloud", C.c_int32)]


KERNELS = ("k_cloud_keys", "k_cloud_count", "k_cloud_scan", "k_cloud_scatter", "k_cloud_runs", "k_cloud_buckets", "k_cloud_emit", "k_cloud_view",
           "k_cloud_place", "k_cloud_fuse")
MAX_HIST = 2048
MAX_SCANS = 256
DBG_SCAN_DS, DBG_SCAN_WORLD, DBG_FUSED = 0, 1, 2
WG_POINTS = 4096                   # the points one workgroup of the counting sort owns (csrc/vilcloud.hip: VC_WG_PTS)
ERR_INVALID_ARGUMENT, ERR_DEVICE, ERR_CAPACITY = -1, -2, -7
_FP = C.POINTER(C.c_float)


class CloudError(RowError):
    pass


def default_options(cdll, **kw):
    """vcloud_default_options, then the keyword overrides."""
    o = VcloudOptions()
    f = cdll.vcloud_default_options; f.restype = None
    f(C.byref(o))
    for k, v in kw.items():
        if k not in dict(VcloudOptions._fields_):
            raise TypeError("vcloud_options has no field %r" % k)
        setattr(o, k, v)
    return o


class DepthCloud(RowHandle):
    ERROR, KERNELS = CloudError, KERNELS

    def __init__(self, cdll, max_scan_points=1 << 15, max_scans=32, device=0):
        super().__init__(cdll, "vcloud_")
        self.max_scan_points, self.max_scans = max_scan_points, max_scans
        self._create(C.c_int32(device), C.c_int32(max_scan_points), C.c_int32(max_scans))

    def reset(self):
        self._call("reset")

    def filter(self, xyzi, leaf, hist_size=512):
        """Filter A alone: n x 4 float32 in, the centroids in emission order out."""
        xyzi = np.ascontiguousarray(xyzi, np.float32).reshape(-1, 4)
        n = len(xyzi)
        out = np.zeros((max(1, n), 4), np.float32); m = C.c_int32(0)
        self._call("filter", C.c_int32(n), xyzi.ctypes.data_as(_FP), C.c_float(leaf), C.c_int32(hist_size), out.ctypes.data_as(_FP), C.c_int32(n), C.byref(m))
        return out[:m.value].copy()

    def push_scan(self, stamp, lidar_to_world, xyzi, opts=None):
        """One accepted scan: float32 3 x 4 lidar_to_world, n x 4 raw points in the sensor frame.  Returns the VcloudSummary."""
        m = np.ascontiguousarray(lidar_to_world, np.float32).reshape(12)
        xyzi = np.ascontiguousarray(xyzi, np.float32).reshape(-1, 4)
        s = VcloudSummary()
        self._call("push_scan", C.c_double(stamp), m.ctypes.data_as(_FP), C.c_int32(len(xyzi)), xyzi.ctypes.data_as(_FP), C.byref(opts) if opts is not None else None, C.byref(s))
        return s

    def _read(self, name, *args):
        n = C.c_int32(0)
        st = self._f(name)(self.ctx, *args, None, C.c_int32(0), C.byref(n))                     # capacity 0: the status is "invalid" unless there is nothing, n is set
        if n.value == 0:
            self._chk(name, st)
        out = np.zeros((max(1, n.value), 4), np.float32)
        self._call(name, *args, out.ctypes.data_as(_FP), C.c_int32(n.value), C.byref(n))
        return out[:n.value]

    def read_cloud(self):
        """The depth cloud, n_cloud x 4 float32."""
        return self._read("read_cloud")

    def debug_read(self, stage):
        """One of DBG_SCAN_DS, DBG_SCAN_WORLD, DBG_FUSED of the last push_scan."""
        return self._read("debug_read", C.c_int32(stage))

    def publish(self, depthreg):
        """Make the depth cloud the resident cloud of a depthreg.DepthReg on the same device, without leaving the device."""
        self._call("publish", depthreg.ctx)


def counts(s):
    """The seven counts of a VcloudSummary as a tuple, in the struct's order."""
    return (s.n_raw, s.n_scan_ds, s.n_in_view, s.n_scans, s.n_popped, s.n_fused, s.n_cloud)
