"""ctypes layer over include/vilsc.h (Scan Context place recognition, SCManager of lidar_mapping) + a synthetic world and trajectory for it.

`ScanContext(cdll)` drives csrc/libvilsolve.so (HIP; needs a GPU, no CPU fallback).  The only CPU restatement is tests/scancontext_ref.py.
"""
import ctypes as C

import numpy as np

from ._row import RowError, RowHandle

NUM_RING, NUM_SECTOR = 20, 60
MAX_CANDIDATES = 16
MODE_REFERENCE, MODE_EXHAUSTIVE = 0, 1
KERNELS = ("k_sc_bin", "k_sc_finish", "k_sc_cand", "k_sc_select", "k_sc_score", "k_sc_decide")
_FP, _DP, _IP = C.POINTER(C.c_float), C.POINTER(C.c_double), C.POINTER(C.c_int32)


class VscConfig(C.Structure):
    _fields_ = [("lidar_height", C.c_double), ("max_radius", C.c_double), ("dist_thres", C.c_double), ("search_ratio", C.c_double),
                ("num_exclude_recent", C.c_int32), ("num_candidates", C.c_int32)]


class VscResult(C.Structure):
    _fields_ = [("min_dist", C.c_double), ("loop_id", C.c_int32), ("nn_idx", C.c_int32), ("nn_align", C.c_int32), ("n_searched", C.c_int32),
                ("yaw_diff_rad", C.c_float), ("pad", C.c_int32)]


class ScanContextError(RowError):
    pass


def default_config(cdll, **kw):
    cfg = VscConfig()
    f = cdll.vsc_default_config; f.restype = None
    f(C.byref(cfg))
    for k, v in kw.items():
        if k not in dict(VscConfig._fields_):
            raise AttributeError("vsc_config has no field %r" % k)
        setattr(cfg, k, v)
    return cfg


class ScanContext(RowHandle):
    """The resident database.  Keyword arguments beyond the sizes are fields of vsc_config (lidar_height, max_radius, dist_thres,
    search_ratio, num_exclude_recent, num_candidates)."""
    ERROR, KERNELS = ScanContextError, KERNELS

    def __init__(self, cdll, max_entries=4096, max_points=1 << 17, device=0, **config):
        super().__init__(cdll, "vsc_")
        self.cfg = default_config(cdll, **config)
        self._scored = 0
        self._create(C.c_int32(device), C.c_int32(max_entries), C.c_int32(max_points), C.byref(self.cfg))

    def push_scan(self, xyzi):
        """xyzi: n x 4 float32, sensor frame.  Returns the new entry's id."""
        xyzi = np.ascontiguousarray(xyzi, np.float32).reshape(-1, 4)
        out = C.c_int32(-1)
        self._call("push_scan", C.c_int32(len(xyzi)), xyzi.ctypes.data_as(_FP), C.byref(out))
        return out.value

    def push_descriptor(self, desc):
        """desc: 20 x 60 float32 (ring, sector)."""
        desc = np.ascontiguousarray(desc, np.float32)
        assert desc.shape == (NUM_RING, NUM_SECTOR)
        out = C.c_int32(-1)
        self._call("push_descriptor", desc.ctypes.data_as(_FP), C.byref(out))
        return out.value

    def detect(self, mode=MODE_REFERENCE, n_search=-1):
        """The newest entry against entries [0, n_search); n_search < 0: count - num_exclude_recent.  Returns a VscResult."""
        r = VscResult()
        self._call("detect", C.c_int32(mode), C.c_int32(n_search), C.byref(r))
        self._scored = 0 if r.n_searched == 0 else (min(self.cfg.num_candidates, r.n_searched) if mode == MODE_REFERENCE else r.n_searched)
        return r

    def count(self):
        return self._f("count")(self.ctx)

    def reset(self):
        self._call("reset")
        self._scored = 0

    def read_entry(self, i):
        """(descriptor 20 x 60 float32, ring key 20 float32, sector key 60 float64) of entry i."""
        desc = np.zeros((NUM_RING, NUM_SECTOR), np.float32); rk = np.zeros(NUM_RING, np.float32); sk = np.zeros(NUM_SECTOR, np.float64)
        self._call("read_entry", C.c_int32(i), desc.ctypes.data_as(_FP), rk.ctypes.data_as(_FP), sk.ctypes.data_as(_DP))
        return desc, rk, sk

    def debug_read(self):
        """(dist float64, shift int32, candidates int32) per scored entry of the last detect, in the order the decision visited them."""
        n = self._scored
        dist = np.zeros(max(1, n)); shift = np.zeros(max(1, n), np.int32); cand = np.zeros(max(1, n), np.int32)
        self._call("debug_read", C.c_int32(n), dist.ctypes.data_as(_DP), shift.ctypes.data_as(_IP), cand.ctypes.data_as(_IP))
        return dist[:n], shift[:n], cand[:n]


def rot_z(yaw):
    """Rotation by `yaw` radians about z."""
    c, s = np.cos(yaw), np.sin(yaw)
    return np.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]])


def yaw_of_align(nn_align):
    """The yaw of the query's sensor minus the yaw of the matched entry's, in radians, to the width of a sector (vilsc.h, SIGN OF nn_align)."""
    return -np.deg2rad(6.0 * nn_align)


# ---- synthetic world: seven walled yards of different sizes, a 16-ring LiDAR at the centre of one of them per keyframe -------------------
# Scan Context's distance is a mean of column cosines; between two arbitrary places it is a noisy value around 0.6 .. 0.9 whose minimum over
# 60 shifts and many entries reaches well below that.  This world makes the separation a matter of construction instead: yard k is a
# square of half-width ROOM_HALF[k], its walls lie at ranges [a, a sqrt 2] from the centre, and the half-widths are chosen so that these
# intervals fall into DISJOINT sets of the 20 rings of 1.5 m (SCENE_RADIUS / 20).  Two different yards then share no occupied ring, every
# column dot product is 0 and the distance is 1.  (A beam that passes over a low segment next to a corner can meet the end of the
# neighbouring wall a little farther out: two yards of neighbouring sizes may share a ring in a few corner columns, and the distance is
# then a little below 1.)  Each wall is a row of five segments of different heights, about half of them
# ending below the sensor: with SCENE_LIDAR_HEIGHT = 0 (scans in a levelled frame at sensor height, the case Scancontext.h:80 names) the
# descriptor has both signs, which is what makes the yaw observable -- a column with one occupied ring has cosine +-1 whatever its height --
# and breaks the square's 90 degree symmetry.  The beams span -3 .. +15 degrees: the floor is met 32 m out, beyond SCENE_RADIUS.
SCENE_RADIUS = 30.0
SCENE_LIDAR_HEIGHT = 0.0
SENSOR_HEIGHT = 1.7
EDGE_MARGIN_DEG = 1e-3
ROOM_HALF = (1.6, 3.1, 4.6, 7.6, 12.1, 18.1, 27.1)         # walls in rings {2}, {3}, {4, 5}, {6..8}, {9..12}, {13..18}, {19, 20}
WALL_SEGMENTS, WALL_THICKNESS = 5, 0.2


def theta_deg(x, y):
    """xy2theta of the contract on float32 arrays: the float quotient, atan in double, the result rounded to float."""
    x = np.asarray(x, np.float32); y = np.asarray(y, np.float32)
    k = 180.0 / np.pi
    with np.errstate(divide="ignore", invalid="ignore"):
        q1 = k * np.arctan((y / x).astype(np.float64))
        q2 = 180.0 - k * np.arctan((y / (-x)).astype(np.float64))
        q3 = 180.0 + k * np.arctan((y / x).astype(np.float64))
        q4 = 360.0 - k * np.arctan(((-y) / x).astype(np.float64))
    out = np.where((x >= 0) & (y >= 0), q1, np.where((x < 0) & (y >= 0), q2, np.where((x < 0) & (y < 0), q3, q4)))
    return out.astype(np.float32)


def keep_off_sector_edges(xyzi, margin=EDGE_MARGIN_DEG):
    """Drops the points whose theta lies within `margin` degrees of a multiple of 6 degrees (about 30 float ulps at 360): a last-bit
    difference between two implementations of atan can then not move a point across a sector edge."""
    th = theta_deg(xyzi[:, 0], xyzi[:, 1]).astype(np.float64)
    r = np.abs(th / 6.0 - np.round(th / 6.0)) * 6.0
    return xyzi[r >= margin]


def make_room(a, rng):
    """The wall segments of a yard of half-width a centred on the origin, as axis-aligned boxes (lo, hi), n x 3 each, floor at z = 0.  A
    segment's top lies 0.01 a .. 0.045 a below the sensor or 0.03 a .. 0.22 a above it (the lowest beam reaches 0.052 a below it at the
    wall, the highest 0.27 a above)."""
    lo, hi = [], []
    edges = np.linspace(-a - WALL_THICKNESS, a + WALL_THICKNESS, WALL_SEGMENTS + 1)
    for axis in (0, 1):
        for side in (-1.0, 1.0):
            for k in range(WALL_SEGMENTS):
                top = SENSOR_HEIGHT + (rng.uniform(0.03, 0.22) if rng.random() < 0.5 else -rng.uniform(0.01, 0.045)) * a
                l, h = np.zeros(3), np.zeros(3)
                l[axis], h[axis] = (a, a + WALL_THICKNESS) if side > 0 else (-a - WALL_THICKNESS, -a)
                l[1 - axis], h[1 - axis] = edges[k], edges[k + 1]
                h[2] = top
                lo.append(l); hi.append(h)
    return np.array(lo), np.array(hi)


def make_world(seed=0):
    """One (lo, hi) per yard of ROOM_HALF.  The yards stand far apart: from inside one, nothing of another lies within SCENE_RADIUS."""
    rng = np.random.default_rng(1000 + seed)
    return [make_room(a, rng) for a in ROOM_HALF]


def lidar_scan(room, R, t, rng, rings=16, az=600, noise=0.01, lower=-3.0, upper=15.0):
    """Points [x y z 0] in the sensor frame (float32) of a spinning LiDAR at pose (R, t) in the yard's frame: per beam the nearest of the
    floor z = 0 and the wall segments; a beam that passes over the wall returns nothing."""
    lo, hi = room
    el = np.deg2rad(np.linspace(lower, upper, rings)); a = np.linspace(0, 2 * np.pi, az, endpoint=False)
    d = np.stack([np.outer(np.cos(el), np.cos(a)).ravel(), np.outer(np.cos(el), np.sin(a)).ravel(), np.outer(np.sin(el), np.ones_like(a)).ravel()], axis=1)
    dw = d @ np.asarray(R, np.float64).T
    t = np.asarray(t, np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        best = np.where(dw[:, 2] < 0, -t[2] / dw[:, 2], np.inf)                                    # the floor
        t0 = (lo[None] - t) / dw[:, None, :]; t1 = (hi[None] - t) / dw[:, None, :]                 # slabs: rays x boxes x 3
        near = np.minimum(t0, t1).max(axis=2); far = np.maximum(t0, t1).min(axis=2)
        box = np.where((near <= far) & (near > 0), near, np.inf).min(axis=1)
    best = np.minimum(best, box)
    ok = np.isfinite(best)
    r = best[ok] + rng.normal(0, noise, int(ok.sum()))
    pts = d[ok] * r[:, None]
    return np.concatenate([pts, np.zeros((len(pts), 1))], axis=1).astype(np.float32)


N_PLACES, N_REVISITS = len(ROOM_HALF), 4
PLACE_ORDER = (3, 0, 5, 2, 6, 1, 4)                        # the yard of keyframe k
REVISIT_YAW_DEG = (90.0, 138.0, 222.0, 300.0)


def make_trajectory(seed=0):
    """11 keyframes: the seven yards in PLACE_ORDER, each from within 4 cm of its centre, then the first four again, from another spot
    within 4 cm of the centre and with the yaw changed by REVISIT_YAW_DEG plus up to one degree.  Returns [(R, t, yard, revisit_of)],
    revisit_of = the first visit's keyframe or -1; t is in the yard's own frame.  The sensor stays level (Scan Context assumes it) and
    SENSOR_HEIGHT above the floor."""
    rng = np.random.default_rng(2000 + seed)
    spot = lambda: np.array([rng.uniform(-0.04, 0.04), rng.uniform(-0.04, 0.04), SENSOR_HEIGHT])
    poses = [(rng.uniform(-np.pi, np.pi), spot(), PLACE_ORDER[k], -1) for k in range(N_PLACES)]
    for k in range(N_REVISITS):
        poses.append((poses[k][0] + np.deg2rad(REVISIT_YAW_DEG[k] + rng.uniform(-1.0, 1.0)), spot(), PLACE_ORDER[k], k))
    return [(rot_z(yaw), t, yard, rev) for yaw, t, yard, rev in poses]


def make_scene(seed=0, az=600, rings=16):
    """(scans, poses, revisit_of): one scan per keyframe of make_trajectory in the world of make_world, kept off the sector edges; poses
    are (R, t) in the keyframe's yard.  Scan Context is to be configured with max_radius = SCENE_RADIUS and lidar_height =
    SCENE_LIDAR_HEIGHT for it."""
    traj = make_trajectory(seed)
    world = make_world(seed)
    rng = np.random.default_rng(3000 + seed)
    scans = [keep_off_sector_edges(lidar_scan(world[yard], R, t, rng, rings=rings, az=az)) for R, t, yard, _ in traj]
    return scans, [(R, t) for R, t, _, _ in traj], [rev for _, _, _, rev in traj]
