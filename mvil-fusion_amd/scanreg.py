"""ctypes layer over include/vilscan.h (LOAM feature extraction of a raw LiDAR scan, the stage upstream of mapreg) + a raw-scan
generator for the synthetic room.

`ScanReg(cdll)` drives csrc/libvilsolve.so (HIP; needs a GPU, no CPU fallback).  The only CPU restatement is tests/scanreg_ref.py.
"""
import ctypes as C

import numpy as np

from ._row import RowError, RowHandle


class VscanConfig(C.Structure):
    _fields_ = [("num_rings", C.c_int32), ("lower_bound_deg", C.c_float), ("upper_bound_deg", C.c_float), ("num_scan_subregions", C.c_int32),
                ("num_curvature_regions", C.c_int32), ("surf_curv_th", C.c_float), ("max_corner_sharp", C.c_int32), ("max_corner_less_sharp", C.c_int32),
                ("max_surf_flat", C.c_int32), ("less_flat_filter_size", C.c_float), ("uneven", C.c_int32)]


class VscanCloud(C.Structure):
    _fields_ = [("xyzi", C.POINTER(C.c_float)), ("capacity", C.c_int32), ("count", C.c_int32)]


class VscanResult(C.Structure):
    _fields_ = [("cloud", VscanCloud), ("ring_table", C.POINTER(C.c_int32)), ("ring_capacity", C.c_int32), ("num_rings", C.c_int32),
                ("labels", C.POINTER(C.c_int8)), ("label_capacity", C.c_int32), ("n_less_flat_raw", C.c_int32),
                ("corner_sharp", VscanCloud), ("corner_less_sharp", VscanCloud), ("surf_flat", VscanCloud), ("surf_less_flat", VscanCloud)]


KERNELS = ("k_scan_ring_id", "k_scan_ring_sort", "k_scan_features", "k_scan_gather")
MAX_RING_POINTS = 4096
CLOUDS = ("cloud", "corner_sharp", "corner_less_sharp", "surf_flat", "surf_less_flat")


class ScanRegError(RowError):
    pass


class Features:
    """What one vscan_extract call returns: cloud / corner_sharp / corner_less_sharp / surf_flat / surf_less_flat (float32 n x 4),
    ring_table (int32 rings x [start, count]), labels (int8 per point of cloud), n_less_flat_raw."""


def default_config(cdll, **kw):
    cfg = VscanConfig()
    cdll.vscan_default_config.restype = None
    cdll.vscan_default_config(C.byref(cfg))
    for k, v in kw.items():
        if k not in dict(VscanConfig._fields_):
            raise AttributeError("vscan_config has no field %r" % k)
        setattr(cfg, k, v)
    return cfg


class ScanReg(RowHandle):
    ERROR, KERNELS = ScanRegError, KERNELS

    def __init__(self, cdll, cfg=None, max_points=1 << 17, device=0):
        super().__init__(cdll, "vscan_")
        self.cfg = cfg or default_config(cdll)
        self.max_points = max_points
        self._create(C.c_int32(device), C.byref(self.cfg), C.c_int32(max_points))

    def capacities(self, n):
        """The largest count each output of an n-point scan can have."""
        c = self.cfg
        rs = c.num_rings * c.num_scan_subregions
        return dict(cloud=n, corner_sharp=rs * c.max_corner_sharp, corner_less_sharp=rs * c.max_corner_less_sharp, surf_flat=rs * c.max_surf_flat, surf_less_flat=n)

    def extract(self, xyzi, capacities=None):
        """xyzi: n x 4 float32 in arrival order.  capacities: overrides of `capacities(n)` (tests of the error path)."""
        xyzi = np.ascontiguousarray(xyzi, np.float32).reshape(-1, 4)
        n = len(xyzi)
        cap = self.capacities(n)
        cap.update(capacities or {})
        res = VscanResult()
        buf = {}
        for name in CLOUDS:
            buf[name] = np.zeros((max(1, cap[name]), 4), np.float32)
            cl = getattr(res, name)
            cl.xyzi = buf[name].ctypes.data_as(C.POINTER(C.c_float)); cl.capacity = cap[name]
        table = np.zeros((self.cfg.num_rings, 2), np.int32); labels = np.zeros(max(1, cap.get("labels", n)), np.int8)
        res.ring_table = table.ctypes.data_as(C.POINTER(C.c_int32)); res.ring_capacity = cap.get("rings", self.cfg.num_rings)
        res.labels = labels.ctypes.data_as(C.POINTER(C.c_int8)); res.label_capacity = cap.get("labels", n)
        self._call("extract", C.c_int32(n), xyzi.ctypes.data_as(C.POINTER(C.c_float)), C.byref(res))
        out = Features()
        for name in CLOUDS:
            setattr(out, name, buf[name][:getattr(res, name).count].copy())
        out.ring_table = table; out.labels = labels[:res.cloud.count].copy(); out.n_less_flat_raw = res.n_less_flat_raw
        return out


# ---- raw scan of a spinning LiDAR in the 20 x 20 x 5 m room of mapreg.make_map / vgicp.scan ---------------------------------
RING_MARGIN_DEG = 0.2


def ring_elevations(rings=16, lower=-15.0, upper=15.0):
    """Beam elevations (degrees): the centres of the rings of ElevationToRing, half a ring spacing from either boundary."""
    return np.linspace(lower, upper, rings) if rings > 1 else np.array([0.5 * (lower + upper)])


def make_raw_scan(R, t, seed=0, rings=16, az=1800, lower=-15.0, upper=15.0, noise=0.01):
    """The scan a `rings`-beam LiDAR at world pose (R, t) takes of the room: float32 [x y z intensity] in the sensor frame, in FIRING order
    (azimuth-major, the rings interleaved), range noise along the beam only -- so every elevation stays a beam's, at least RING_MARGIN_DEG
    from a ring boundary, and a last-bit difference in atan2f cannot move a point to another ring.  Intensities are positive: one band
    per wall, as mapreg.make_map's surf points."""
    el = ring_elevations(rings, lower, upper)
    if rings > 1 and 0.5 * (upper - lower) / (rings - 1) < RING_MARGIN_DEG + 1e-3:
        raise ValueError("ring spacing leaves less than %.1f degrees to a ring boundary" % RING_MARGIN_DEG)
    rng = np.random.default_rng(seed)
    lo, hi = np.array([-10.0, -10.0, -1.5]), np.array([10.0, 10.0, 3.5])
    a = np.linspace(0, 2 * np.pi, az, endpoint=False)
    e = np.deg2rad(el)
    A, E = np.meshgrid(a, e, indexing="ij")                            # azimuth-major
    d = np.stack([np.cos(E) * np.cos(A), np.cos(E) * np.sin(A), np.sin(E)], axis=-1).reshape(-1, 3)
    dw = d @ np.asarray(R, np.float64).T
    with np.errstate(divide="ignore", invalid="ignore"):
        t_lo, t_hi = (lo - t) / dw, (hi - t) / dw
    tt = np.where(dw > 0, t_hi, t_lo)
    axis = np.argmin(tt, axis=1); r = tt[np.arange(len(tt)), axis]
    side = (dw[np.arange(len(dw)), axis] > 0).astype(np.int64)
    r = r + rng.normal(0, noise, len(r))
    inten = 10.0 * (2 * axis + side) + rng.uniform(0.05, 5.0, len(r))
    return np.concatenate([d * r[:, None], inten[:, None]], axis=1).astype(np.float32)
