"""ctypes layer over include/vilgmap.h: the global map of lidar_mapping resident on the device -- keyed scans, voxel-thinned insertion
(InsertPoints), the registration reference cut from the map (ApproxNearestNeighbors, OcTree and IkdTree variants) and the rebuild from
the keyed scans at optimised poses.

`GlobalMap(cdll)` drives csrc/libvilsolve.so (HIP; needs a GPU, no CPU fallback).  The only CPU restatement is tests/globalmap_ref.py.
"""
import ctypes as C

import numpy as np

from ._row import RowError, RowHandle

MAX_K = 64
VOXEL_LIMIT = 1 << 20
REF_RADIUS, REF_KNN = 0, 1
MODES = {"radius": REF_RADIUS, "knn": REF_KNN}
# the slots of vgmap_profile_read; "grid" is the rebuild of the search grid (three kernels of vil_knn.hpp), the others are DEVICE_KERNELS
KERNELS = ("k_gmap_xform", "k_gmap_claim", "k_gmap_survive", "k_gmap_scan", "k_gmap_append", "k_gmap_wipe", "grid", "k_gmap_radius", "k_gmap_thin", "k_gmap_pick", "k_gmap_emit",
           "k_gmap_unclaim", "k_gmap_knn")
DEVICE_KERNELS = tuple(k for k in KERNELS if k != "grid")
_FP, _DP, _IP = C.POINTER(C.c_float), C.POINTER(C.c_double), C.POINTER(C.c_int32)


class VgmapConfig(C.Structure):
    _fields_ = [("max_map_points", C.c_int32), ("max_scan_points", C.c_int32), ("max_keys", C.c_int32), ("max_keyed_points", C.c_int32), ("max_ref_points", C.c_int32),
                ("map_resolution", C.c_float), ("origin", C.c_double * 3)]


class VgmapRefOptions(C.Structure):
    _fields_ = [("mode", C.c_int32), ("k", C.c_int32), ("radius", C.c_double), ("ref_resolution", C.c_float), ("max_dist", C.c_float)]


class GlobalMapError(RowError):
    pass


def _defaults(cdll, name, struct, kw):
    o = struct()
    f = getattr(cdll, name); f.restype = None
    f(C.byref(o))
    for k, v in kw.items():
        if k not in dict(struct._fields_):
            raise AttributeError("%s has no field %r" % (struct.__name__, k))
        if k == "origin":
            o.origin[:] = [float(x) for x in v]
        else:
            setattr(o, k, v)
    return o


def default_config(cdll, **kw):
    """vgmap_default_config; keyword arguments set fields of vgmap_config."""
    return _defaults(cdll, "vgmap_default_config", VgmapConfig, kw)


def default_ref_options(cdll, **kw):
    """vgmap_default_ref_options; keyword arguments set fields of vgmap_ref_options (mode: "radius" | "knn" or the constant)."""
    if "mode" in kw:
        kw = dict(kw, mode=MODES.get(kw["mode"], kw["mode"]))
    return _defaults(cdll, "vgmap_default_ref_options", VgmapRefOptions, kw)


def _xyz(a):
    return np.ascontiguousarray(a, np.float32).reshape(-1, 3)


def _T(T):
    return np.ascontiguousarray(T, np.float64).reshape(-1)


class GlobalMap(RowHandle):
    """The resident map.  config: a VgmapConfig (default_config) or None for the defaults with the keyword arguments applied."""
    ERROR, KERNELS = GlobalMapError, KERNELS

    def __init__(self, cdll, config=None, device=0, **kw):
        super().__init__(cdll, "vgmap_")
        self.config = config if config is not None else default_config(cdll, **kw)
        self._create(C.c_int32(device), C.byref(self.config))

    def add_scan(self, key, xyz):
        xyz = _xyz(xyz)
        self._call("add_scan", C.c_int32(key), C.c_int32(len(xyz)), xyz.ctypes.data_as(_FP))

    def insert(self, xyz, T):
        xyz, T = _xyz(xyz), _T(T)
        self._call("insert", C.c_int32(len(xyz)), xyz.ctypes.data_as(_FP), T.ctypes.data_as(_DP))

    def insert_key(self, key, T):
        T = _T(T)
        self._call("insert_key", C.c_int32(key), T.ctypes.data_as(_DP))

    def reference(self, xyz, T, T_out=None, mode=None, options=None, **kw):
        """The reference cloud for the query xyz (sensor frame) at pose T: (ref_xyz n_ref x 3 float32, ref_idx n_ref int32).  options: a
        VgmapRefOptions, or None for the defaults with mode and the keyword arguments applied.  T_out: the hand-over transform or None."""
        xyz, T = _xyz(xyz), _T(T)
        if options is None:
            options = default_ref_options(self.lib, **(dict(kw, mode=mode) if mode is not None else kw))
        To = _T(T_out) if T_out is not None else None
        cap = self.config.max_ref_points
        out = np.zeros((cap, 3), np.float32); idx = np.zeros(cap, np.int32); n = C.c_int32(0)
        self._call("reference", C.c_int32(len(xyz)), xyz.ctypes.data_as(_FP), T.ctypes.data_as(_DP), C.byref(options), To.ctypes.data_as(_DP) if To is not None else C.cast(None, _DP),
                   C.byref(n), out.ctypes.data_as(_FP), idx.ctypes.data_as(_IP))
        return out[:n.value].copy(), idx[:n.value].copy()

    def rebuild(self, keys, Ts):
        keys = np.ascontiguousarray(keys, np.int32).reshape(-1); Ts = _T(Ts)
        if len(Ts) != 16 * len(keys):
            raise ValueError("rebuild takes one 4 x 4 per key")
        self._call("rebuild", C.c_int32(len(keys)), keys.ctypes.data_as(_IP), Ts.ctypes.data_as(_DP))

    def size(self):
        """(n_map, n_keys, n_keyed_points)"""
        a, b, c = C.c_int32(0), C.c_int32(0), C.c_int32(0)
        self._call("size", C.byref(a), C.byref(b), C.byref(c))
        return a.value, b.value, c.value

    def points(self, first=0, n=None):
        """Map points first .. first + n - 1 (all from `first` by default) as n x 3 float32."""
        if n is None:
            n = self.size()[0] - first
        out = np.zeros((max(n, 0), 3), np.float32)
        if n > 0:
            self._call("get_points", C.c_int32(first), C.c_int32(n), out.ctypes.data_as(_FP))
        return out

    def clear(self):
        self._call("clear")
