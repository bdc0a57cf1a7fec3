"""ctypes layer over include/vildepth.h (LiDAR depth association of visual features, DepthRegister::get_depth of the feature tracker)
+ the host-side matrices and a synthetic scene for it.

`DepthReg(cdll)` drives csrc/libvilsolve.so (HIP; needs a GPU, no CPU fallback).  The only CPU restatement is tests/depthreg_ref.py.
"""
import ctypes as C

import numpy as np

from . import scanreg
from ._row import RowError, RowHandle
from .vgicp import _rot


class VdepthSummary(C.Structure):
    _fields_ = [("n_cloud", C.c_int32), ("n_in_view", C.c_int32), ("n_sphere", C.c_int32), ("n_with_depth", C.c_int32)]


KERNELS = ("k_depth_project", "k_depth_compact", "k_depth_query")
BINS = 360
MIN_SPHERE = 10
_FP = C.POINTER(C.c_float)


class DepthRegError(RowError):
    pass


class Depths:
    """What one vdepth_register call returns: depth (float32 n_feat, -1 = none), n_cloud, n_in_view, n_sphere, n_with_depth."""


class DepthReg(RowHandle):
    ERROR, KERNELS = DepthRegError, KERNELS

    def __init__(self, cdll, max_cloud_points=1 << 17, max_features=1024, device=0):
        super().__init__(cdll, "vdepth_")
        self.max_cloud_points, self.max_features = max_cloud_points, max_features
        self._last = (0, 0)
        self._create(C.c_int32(device), C.c_int32(max_cloud_points), C.c_int32(max_features))

    def set_cloud(self, xyzi):
        """xyzi: n x 4 float32, world frame; stays on the device until the next set_cloud."""
        xyzi = np.ascontiguousarray(xyzi, np.float32).reshape(-1, 4)
        self._call("set_cloud", C.c_int32(len(xyzi)), xyzi.ctypes.data_as(_FP))

    def register(self, world_to_lidar, lidar_to_view, feat_xyz, depth_out=None):
        """The two float32 3 x 4 matrices of view_matrices and n_feat x 3 features.  depth_out: a float32 array to write into (tests of
        the error path); a fresh one otherwise."""
        m1 = np.ascontiguousarray(world_to_lidar, np.float32).reshape(12); m2 = np.ascontiguousarray(lidar_to_view, np.float32).reshape(12)
        feat = np.ascontiguousarray(feat_xyz, np.float32).reshape(-1, 3)
        n = len(feat)
        depth = depth_out if depth_out is not None else np.zeros(max(1, n), np.float32)
        s = VdepthSummary()
        self._call("register", m1.ctypes.data_as(_FP), m2.ctypes.data_as(_FP), C.c_int32(n), feat.ctypes.data_as(_FP), depth.ctypes.data_as(_FP), C.byref(s))
        out = Depths()
        out.depth = depth[:n].copy()
        out.n_cloud, out.n_in_view, out.n_sphere, out.n_with_depth = s.n_cloud, s.n_in_view, s.n_sphere, s.n_with_depth
        self._last = (s.n_sphere, n)
        return out

    def debug_read(self):
        """(sphere n_sphere x 4 [x y z range] in emission order, nn3 n_feat x 3) of the last register."""
        ns, nf = self._last
        sphere = np.zeros((max(1, ns), 4), np.float32); nn3 = np.zeros((max(1, nf), 3), np.int32)
        self._call("debug_read", sphere.ctypes.data_as(_FP), C.c_int32(ns), nn3.ctypes.data_as(C.POINTER(C.c_int32)))
        return sphere[:ns], nn3[:nf]


# ---- the host side of get_depth: the two matrices -----------------------------------------------------------------------------
# Tlc_ (feature_tracker.h:134-138): camera axes (x right, y down, z forward) to the LiDAR convention (x forward, y left, z up)
TLC = np.array([[0.0, 0.0, 1.0, 0.0], [-1.0, 0.0, 0.0, 0.0], [0.0, -1.0, 0.0, 0.0], [0.0, 0.0, 0.0, 1.0]])


def _h(R, t):
    T = np.eye(4); T[:3, :3] = np.asarray(R, np.float64); T[:3, 3] = np.asarray(t, np.float64)
    return T


def view_matrices(R_wl, t_wl, R_lc, t_lc):
    """(world_to_lidar, lidar_to_view), float32 3 x 4.  (R_wl, t_wl): the LiDAR's pose in the world at the image's time, p_w = R_wl p_l +
    t_wl, so world_to_lidar is its inverse (transNow.inverse(), :132).  (R_lc, t_lc): the camera's pose in the LiDAR frame (TransFormLC),
    so lidar_to_view = Tlc_ * TransFormLC.inverse() (:140).  Built in float64 and rounded once; the reference builds them in float on the
    host as well, and whatever it builds is what vdepth_register is given."""
    m1 = np.linalg.inv(_h(R_wl, t_wl))[:3]
    m2 = (TLC @ np.linalg.inv(_h(R_lc, t_lc)))[:3]
    return np.ascontiguousarray(m1, np.float32), np.ascontiguousarray(m2, np.float32)


# ---- synthetic scene: the 20 x 20 x 5 m room of scanreg.make_raw_scan, several scans fused into one world cloud -----------------
EXTRINSIC = (np.array([[0.0, 0.0, 1.0], [-1.0, 0.0, 0.0], [0.0, -1.0, 0.0]]) @ _rot(0.01, -0.012, 0.017), np.array([0.08, -0.02, -0.06]))     # camera in the LiDAR frame
MIN_RANGE = 4.0


def make_scene(R_wl, t_wl, seed=0, n_poses=4, az=300, n_feat=150, half_fov=(0.8, 0.6), rings=16, extrinsic=EXTRINSIC):
    """A world-frame depth cloud and the features of one image taken at LiDAR pose (R_wl, t_wl).

    cloud: `n_poses` 16-ring scans taken around that pose (different heights, pitches and yaws, as a moving sensor accumulates them),
    each moved to the world frame and concatenated; points closer than MIN_RANGE to the viewing position are left out (get_depth only
    returns depths above 3 m).  feat: n_feat x 3 [x y 1], projections of wall points (a dense noise-free scan from the camera's side of
    the sensor) into the camera, inside +-half_fov in normalised coordinates -- wider than the LiDAR's +-15 degrees, so a part of the
    features has no depth.  Returns cloud (n x 4 float32), feat (float32), true_depth (float64, the camera-frame z of each wall point)."""
    rng = np.random.default_rng(seed)
    R_wl = np.asarray(R_wl, np.float64); t_wl = np.asarray(t_wl, np.float64)
    parts = []
    for k in range(n_poses):
        a = rng.uniform(-0.12, 0.12, 2); yaw = rng.uniform(-0.5, 0.5)
        R = R_wl @ _rot(a[1], a[0], yaw); t = t_wl + np.array([rng.uniform(-0.6, 0.6), rng.uniform(-0.6, 0.6), rng.uniform(-0.3, 0.3)])
        s = scanreg.make_raw_scan(R, t, seed=1000 * seed + k, rings=rings, az=az).astype(np.float64)
        w = s[:, :3] @ R.T + t
        parts.append(np.concatenate([w, s[:, 3:]], axis=1))
    cloud = np.concatenate(parts)
    cloud = cloud[np.linalg.norm(cloud[:, :3] - t_wl, axis=1) >= MIN_RANGE]
    # wall points seen from the camera
    R_lc, t_lc = extrinsic
    dense = scanreg.make_raw_scan(R_wl, t_wl, seed=seed, rings=61, az=720, lower=-45.0, upper=45.0, noise=0.0).astype(np.float64)[:, :3]
    pc = (dense - t_lc) @ np.asarray(R_lc, np.float64)                      # R_lc^T (p_l - t_lc)
    keep = (pc[:, 2] > 0.5)
    pc = pc[keep]
    xy = pc[:, :2] / pc[:, 2:3]
    inside = (np.abs(xy[:, 0]) < half_fov[0]) & (np.abs(xy[:, 1]) < half_fov[1])
    pc, xy = pc[inside], xy[inside]
    pick = rng.choice(len(pc), size=n_feat, replace=False)
    feat = np.concatenate([xy[pick], np.ones((n_feat, 1))], axis=1).astype(np.float32)
    return cloud.astype(np.float32), feat, pc[pick, 2].copy()
