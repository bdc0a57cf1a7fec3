"""ctypes layer over include/villmap.h: lidar_mapping's local cube map (process() of localMapping.cpp), resident on the device.

`LocalMap(cdll)` drives csrc/libvilsolve.so (HIP; needs a GPU, no CPU fallback).  The only CPU restatement of the bookkeeping is
tests/localmap_ref.py; the stacks' filter and the registration are the cloud and mapreg rows.
"""
import ctypes as C

import numpy as np

from . import abi
from ._row import RowError, RowHandle
from .mapreg import VmapSummary


class VlmapConfig(C.Structure):
    _fields_ = [("line_res", C.c_float), ("plane_res", C.c_float), ("hist_size", C.c_int32), ("publish_first_frame", C.c_int32), ("cube_length", C.c_double),
                ("cube_height", C.c_double), ("publish_distance", C.c_double), ("publish_frames", C.c_int32), ("max_scan_points", C.c_int32),
                ("max_map_points", C.c_int32), ("reserved", C.c_int32)]


class VlmapSummary(C.Structure):
    _fields_ = [("q_w_curr", C.c_double * 4), ("t_w_curr", C.c_double * 3), ("shift", C.c_int32 * 3), ("n_corner_from_map", C.c_int32), ("n_surf_from_map", C.c_int32),
                ("n_corner_stack", C.c_int32), ("n_surf_stack", C.c_int32), ("aligned", C.c_int32), ("n_corner_added", C.c_int32), ("n_surf_added", C.c_int32),
                ("n_corner_map", C.c_int32), ("n_surf_map", C.c_int32), ("published", C.c_int32), ("frame_count", C.c_int32), ("reserved", C.c_int32),
                ("align", VmapSummary)]


KERNELS = ("k_lmap_gather", "k_lmap_place", "k_lmap_layout", "k_lmap_append", "k_lmap_refilter", "k_lmap_publish")
W, H, D = 11, 11, 7
CUBES = W * H * D
MAX_VALID = 75
CORNER, SURF = 0, 1
DBG_CORNER_STACK, DBG_SURF_STACK, DBG_CORNER_FROM_MAP, DBG_SURF_FROM_MAP, DBG_MATRIX = 0, 1, 2, 3, 4
FRAME_WORLD, FRAME_SENSOR = 0, 1
ERR_INVALID_ARGUMENT, ERR_DEVICE, ERR_CAPACITY = -1, -2, -7
_FP = C.POINTER(C.c_float)
_DP = C.POINTER(C.c_double)


class LocalMapError(RowError):
    pass


def default_config(cdll, **kw):
    """vlmap_default_config, then the keyword overrides."""
    g = VlmapConfig()
    f = cdll.vlmap_default_config; f.restype = None
    f(C.byref(g))
    for k, v in kw.items():
        if k not in dict(VlmapConfig._fields_):
            raise TypeError("vlmap_config has no field %r" % k)
        setattr(g, k, v)
    return g


def summary_counts(s):
    """The integer fields of a VlmapSummary up to frame_count, as a tuple in the struct's order."""
    return (tuple(s.shift), s.n_corner_from_map, s.n_surf_from_map, s.n_corner_stack, s.n_surf_stack, s.aligned, s.n_corner_added, s.n_surf_added,
            s.n_corner_map, s.n_surf_map, s.published, s.frame_count)


class LocalMap(RowHandle):
    ERROR, KERNELS = LocalMapError, KERNELS

    def __init__(self, cdll, device=0, **cfg):
        super().__init__(cdll, "vlmap_")
        self.cfg = default_config(cdll, **cfg)
        self._create(C.c_int32(device), C.byref(self.cfg))

    def reset(self):
        self._call("reset")

    def push_scan(self, solver_ctx, corner, surf, q_wodom, t_wodom, opts=None):
        """One scan: the vil_ctx of a lib.Backend, n x 4 float32 corner and surf feature clouds, the odometry pose (q = x y z w).
        Returns the VlmapSummary."""
        corner = np.ascontiguousarray(corner, np.float32).reshape(-1, 4); surf = np.ascontiguousarray(surf, np.float32).reshape(-1, 4)
        q = np.ascontiguousarray(q_wodom, np.float64).reshape(4); t = np.ascontiguousarray(t_wodom, np.float64).reshape(3)
        opts = opts or abi.default_options(max_iterations=4)                                    # localMapping.cpp:772
        s = VlmapSummary()
        self._call("push_scan", solver_ctx, C.c_int32(len(corner)), corner.ctypes.data_as(_FP), C.c_int32(len(surf)), surf.ctypes.data_as(_FP), q.ctypes.data_as(_DP),
                   t.ctypes.data_as(_DP), C.byref(opts), C.byref(s))
        return s

    def _read(self, name, *args):
        n = C.c_int32(0)
        st = self._f(name)(self.ctx, *args, None, C.c_int32(0), C.byref(n))                     # capacity 0: the status is "invalid" unless there is nothing, n is set
        if n.value == 0:
            self._chk(name, st)
        out = np.zeros((max(1, n.value), 4), np.float32)
        self._call(name, *args, out.ctypes.data_as(_FP), C.c_int32(n.value), C.byref(n))
        return out[:n.value]

    def read_published(self, frame=FRAME_WORLD):
        """The last published local map, n x 4 float32, in FRAME_WORLD or FRAME_SENSOR."""
        return self._read("read_published", C.c_int32(frame))

    def read_cube(self, cls, index):
        """The points of cube `index` (i + 11 j + 121 k) of class CORNER or SURF."""
        return self._read("read_cube", C.c_int32(cls), C.c_int32(index))

    def debug_read(self, stage):
        """One of the DBG_* stages of the last push; DBG_MATRIX comes back as a 3 x 4 float64 matrix (None before the first push)."""
        out = self._read("debug_read", C.c_int32(stage))
        if stage == DBG_MATRIX:
            return out.view(np.float64).reshape(3, 4).copy() if len(out) else None
        return out

    def debug_write_cube(self, cls, index, xyzi):
        """Test hook: cube `index` of class cls holds these raw points, unfiltered, from now on."""
        xyzi = np.ascontiguousarray(xyzi, np.float32).reshape(-1, 4)
        self._call("debug_write_cube", C.c_int32(cls), C.c_int32(index), C.c_int32(len(xyzi)), xyzi.ctypes.data_as(_FP))

    def cubes(self, cls):
        """All 847 cubes of a class, as a list of n x 4 arrays."""
        return [self.read_cube(cls, e) for e in range(CUBES)]
