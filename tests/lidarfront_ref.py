"""Restatements of the de-skew of include/vilfront.h, written from that header's ARITHMETIC CONTRACT (steps 0-9), and the fixtures of
the lidarfront tests.  No GPU.

  deskew_f32   the contract in NumPy float32: every operation one rounded float32 operation, in the order written.  np.arccos and np.sin
               on float32 are NumPy's; the device's acosf and sinf are its own -- that is why the coordinates are compared through
  deskew_mp    the same formulas from the same float inputs at 50 digits (mpmath), unrounded: s, the slerp, the normalisation, the two
               rotations.  The gates of steps 0, 3 and 9 are decisions on float32 values and are taken from deskew_f32.
  room_scan    a 16-ring spinning LiDAR in a small box room, measured while the sensor moves: every column of the scan is cast from the
               pose at its own time, the intensity is ring + scan_period * (relative time) as the scan registration writes it.
"""
import functools

import numpy as np

F = np.float32
EPS32 = float(np.finfo(np.float32).eps)
BRANCHES = ("deviation", "s_neg", "s_hi", "d_min", "d_max", "removed")


def _f(a):
    return np.asarray(a, np.float32)


def _rotate_f32(qw, qx, qy, qz, x, y, z):
    """step 7, Eigen's quaternion * vector"""
    ax = qy * z - qz * y; ay = qz * x - qx * z; az = qx * y - qy * x
    ax = ax + ax; ay = ay + ay; az = az + az
    bx = qy * az - qz * ay; by = qz * ax - qx * az; bz = qx * ay - qy * ax
    return (x + qw * ax) + bx, (y + qw * ay) + by, (z + qw * az) + bz


def time_factor_of(lidar_time_step):
    return F(1.0 / float(lidar_time_step))


def deskew_f32(xyzi, q_wxyz, t, time_factor=None, dmin=0.5, dmax=70.0):
    """Returns (out n x 4 float32 with every point's steps 4-8 result, keep mask, info).  info: per-point boolean arrays named as
    BRANCHES (which gate refused the point; `removed` is step 9), `s` (float32), and the two facts of the motion, `lerp` (the
    absD >= 1 - eps branch) and `d_neg`.  The kept cloud is out[keep]."""
    p = _f(xyzi).reshape(-1, 4)
    qw, qx, qy, qz = (F(v) for v in _f(q_wxyz).reshape(4))
    tx, ty, tz = (F(v) for v in _f(t).reshape(3))
    tf = time_factor_of(0.1) if time_factor is None else F(time_factor)
    x, y, z, w = p[:, 0].copy(), p[:, 1].copy(), p[:, 2].copy(), p[:, 3].copy()
    with np.errstate(all="ignore"):
        deviation = ~((w >= F(-2147483648.0)) & (w < F(2147483648.0)))                              # step 0
        whole = np.trunc(np.where(deviation, F(0), w)).astype(np.float32)                           # (float)(int)w
        dist = np.sqrt(x * x + y * y)                                                               # step 1
        s = tf * (np.where(deviation, F(0), w) - whole)                                             # step 2
        s_neg = ~deviation & (s < F(0))                                                             # step 3
        s_hi = ~deviation & (s.astype(np.float64) > 1.001)
        d_min = ~deviation & (dist.astype(np.float64) < float(dmin))
        d_max = ~deviation & (dist.astype(np.float64) > float(dmax))
        x = x - s * tx; y = y - s * ty; z = z - s * tz                                              # step 4
        d = qw; absD = np.abs(d)                                                                    # step 5
        lerp = bool(absD >= F(1) - F(EPS32))
        if lerp:
            scale0 = F(1) - s; scale1 = s
        else:
            theta = np.arccos(absD); sin_theta = np.sin(theta)
            scale0 = np.sin((F(1) - s) * theta) / sin_theta
            scale1 = np.sin(s * theta) / sin_theta
        d_neg = bool(d < F(0))
        if d_neg:
            scale1 = -scale1
        cw = scale0 + scale1 * qw; cx = -(scale1 * qx); cy = -(scale1 * qy); cz = -(scale1 * qz)      # step 6
        n2 = ((cx * cx + cy * cy) + cz * cz) + cw * cw
        nrm = np.sqrt(n2); pos = n2 > F(0)
        cw = np.where(pos, cw / nrm, cw); cx = np.where(pos, cx / nrm, cx); cy = np.where(pos, cy / nrm, cy); cz = np.where(pos, cz / nrm, cz)
        x, y, z = _rotate_f32(cw, cx, cy, cz, x, y, z)                                              # step 7
        x, y, z = _rotate_f32(qw, qx, qy, qz, x, y, z)
        x = x + tx; y = y + ty; z = z + tz                                                          # step 8
    for a in (x, y, z, s):
        assert a.dtype == np.float32
    gate = deviation | s_neg | s_hi | d_min | d_max
    removed = ~gate & ~(np.isfinite(x) & np.isfinite(y) & np.isfinite(z))                           # step 9
    keep = ~gate & ~removed
    out = np.stack([x, y, z, whole], axis=1).astype(np.float32)
    info = dict(deviation=deviation, s_neg=s_neg, s_hi=s_hi, d_min=d_min, d_max=d_max, removed=removed, s=s, lerp=lerp, d_neg=d_neg)
    return out, keep, info


def deskew_mp(xyzi, q_wxyz, t, time_factor=None, keep=None):
    """Steps 2 and 4-8 at 50 digits for the points of `keep` (default: all): an (n, 3) object array of mpf, None where not evaluated.
    The branch of the slerp is the one the float32 contract takes (absD against 1 - FLT_EPSILON, both float32 values, compared exactly)."""
    import mpmath
    mp = mpmath.mp
    with mpmath.workdps(50):
        mpf = mp.mpf
        p = _f(xyzi).reshape(-1, 4)
        qw, qx, qy, qz = (mpf(float(v)) for v in _f(q_wxyz).reshape(4))
        tx, ty, tz = (mpf(float(v)) for v in _f(t).reshape(3))
        tf = mpf(float(time_factor_of(0.1) if time_factor is None else F(time_factor)))
        absD = abs(qw)
        lerp = absD >= mpf(1) - mpf(EPS32)
        theta = None if lerp else mp.acos(absD)
        sin_theta = None if lerp else mp.sin(theta)

        def rot(w, a, b, c, v):
            x, y, z = v
            ax = b * z - c * y; ay = c * x - a * z; az = a * y - b * x
            ax = ax + ax; ay = ay + ay; az = az + az
            bx = b * az - c * ay; by = c * ax - a * az; bz = a * ay - b * ax
            return (x + w * ax) + bx, (y + w * ay) + by, (z + w * az) + bz

        out = np.full((len(p), 3), None, dtype=object)
        for i in range(len(p)):
            if keep is not None and not keep[i]:
                continue
            x, y, z, w = (mpf(float(v)) for v in p[i])
            s = tf * (w - mpf(int(float(p[i, 3]))))
            v = (x - s * tx, y - s * ty, z - s * tz)
            if lerp:
                s0, s1 = 1 - s, s
            else:
                s0, s1 = mp.sin((1 - s) * theta) / sin_theta, mp.sin(s * theta) / sin_theta
            if qw < 0:
                s1 = -s1
            cw, cx, cy, cz = s0 + s1 * qw, -(s1 * qx), -(s1 * qy), -(s1 * qz)
            n2 = ((cx * cx + cy * cy) + cz * cz) + cw * cw
            if n2 > 0:
                nrm = mp.sqrt(n2); cw, cx, cy, cz = cw / nrm, cx / nrm, cy / nrm, cz / nrm
            v = rot(cw, cx, cy, cz, v)
            v = rot(qw, qx, qy, qz, v)
            out[i] = (v[0] + tx, v[1] + ty, v[2] + tz)
    return out


def abs_err(xyz_f32, exact):
    """|float32 value - 50-digit value| per coordinate as float64 (the difference is taken at 50 digits), for the rows of `exact` that
    were evaluated; xyz_f32 holds the same rows."""
    import mpmath
    out = np.zeros(exact.shape, np.float64)
    with mpmath.workdps(50):
        for i in range(exact.shape[0]):
            for k in range(3):
                out[i, k] = float(abs(mpmath.mpf(float(xyz_f32[i, k])) - exact[i, k]))
    return out


# ---- motions and fixtures ----------------------------------------------------------------------------------------------------------
def quat_z(angle):
    return np.array([np.cos(angle / 2), 0.0, 0.0, np.sin(angle / 2)])


def quat_axis(axis, angle):
    a = np.asarray(axis, np.float64); a = a / np.linalg.norm(a)
    return np.concatenate([[np.cos(angle / 2)], np.sin(angle / 2) * a])


MOTIONS = {
    "generic": (_f(quat_axis((0.2, -0.3, 1.0), 0.06)), _f((0.11, -0.04, 0.02))),                    # absD < 1 - eps, d > 0
    "lerp": (_f((1.0, 0.0, 0.0, 0.0)), _f((0.2, 0.1, -0.05))),                                       # absD >= 1 - eps
    "negative_w": (_f(-quat_axis((0.1, 0.4, 1.0), 0.05)), _f((-0.07, 0.09, 0.01))),                  # d < 0: the same rotation, the other sign
}


def _around_s_limit(tf):
    """Two float32 intensities next to each other in the sequence of s values: the last with (double)s <= 1.001 and the first above."""
    w = F(1.001 / float(tf))
    s_of = lambda v: float(F(tf) * (v - np.trunc(v)))
    while s_of(w) > 1.001:
        w = np.nextafter(w, F(0))
    while s_of(np.nextafter(w, F(1))) <= 1.001:
        w = np.nextafter(w, F(1))
    return w, np.nextafter(w, F(1))


def branch_points(tf=None):
    """Points that between them take every gate of steps 0, 3 and 9, with generic neighbours so that the compaction has work to do."""
    tf = time_factor_of(0.1) if tf is None else F(tf)
    lo, hi = _around_s_limit(tf)
    nan, inf = np.nan, np.inf
    rows = [
        (3.0, 4.0, 0.5, 2.03),                       # kept, generic
        (3.0, 4.0, 0.5, -2.5),                       # s < 0: the truncation goes towards zero
        (3.0, -4.0, 1.0, -3.0),                      # a negative intensity without a fractional part: s = 0, kept
        (1.0, 2.0, -0.5, 7.0),                       # no fractional part: s = 0, kept
        (2.0, 1.0, 0.25, float(lo)),                 # s just below 1.001: kept
        (2.0, 1.0, 0.25, float(hi)),                 # s just above: rejected
        (0.5, 0.0, 0.1, 1.05),                       # distance exactly min: kept
        (float(np.nextafter(F(0.5), F(0))), 0.0, 0.1, 1.05),      # just inside min: rejected
        (0.0, 70.0, 1.0, 4.02),                      # distance exactly max: kept
        (0.0, float(np.nextafter(F(70.0), F(80))), 1.0, 4.02),    # just beyond max: rejected
        (nan, 1.0, 1.0, 5.01),                       # a NaN coordinate passes the gate and is removed
        (1.0, 1.0, nan, 5.01),
        (1.0, 1.0, inf, 5.01),                       # an infinite z: the distance is fine, the result is not finite
        (1.0, 1.0, 1.0, nan),                        # DEVIATION
        (1.0, 1.0, 1.0, 3.0e9),                      # DEVIATION
        (-6.0, 2.5, -1.0, 15.099),                   # kept, generic
    ]
    return np.array(rows, np.float32)


@functools.lru_cache(maxsize=None)
def branch_fixture():
    """[(name, xyzi, q, t)]: the branch points under each of MOTIONS."""
    return tuple((name, branch_points(), q, t) for name, (q, t) in MOTIONS.items())


# ---- a LiDAR in a box room, measured while it moves ----------------------------------------------------------------------------------
ROOM_LO, ROOM_HI = np.array([-3.4, -2.8, -1.1]), np.array([4.2, 3.0, 1.7])
SCAN_PERIOD = 0.1


def _Rz(a):
    c, s = np.cos(a), np.sin(a)
    return np.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]])


def pose_at(tau):
    """The sensor's pose in the room at time tau (seconds): a smooth planar motion with a slow yaw.  Returns (R, c): x_room = R x_sensor + c."""
    return _Rz(0.15 * tau + 0.05 * np.sin(1.3 * tau)), np.array([0.4 * tau + 0.1 * np.sin(0.9 * tau), -0.25 * tau, 0.02 * np.sin(2.0 * tau)])


def room_scan(k, rings=16, az=225, seed=0, noise=0.004):
    """Scan k of the chain, taken over [k, k + 1] * SCAN_PERIOD: (xyzi float32 (rings * az, 4), q, t, guess).  Column j is cast from
    the pose at its own time; intensity = ring + SCAN_PERIOD * j / az.  (q, t): the motion TransformToEnd is given, from the poses at
    the scan's start and end.  guess: previous scan's end frame <- this scan's end frame, row-major 4 x 4 float64."""
    rng = np.random.default_rng(1000 * seed + k)
    t0 = k * SCAN_PERIOD
    el = np.deg2rad(np.linspace(-15, 15, rings)); a = np.linspace(0, 2 * np.pi, az, endpoint=False)
    pts = np.zeros((rings, az, 4))
    for j in range(az):
        rel = j / az
        R, c = pose_at(t0 + rel * SCAN_PERIOD)
        d = np.stack([np.cos(el) * np.cos(a[j]), np.cos(el) * np.sin(a[j]), np.sin(el)], axis=1)
        dw = d @ R.T
        with np.errstate(divide="ignore", invalid="ignore"):
            tt = np.where(dw > 0, (ROOM_HI - c) / dw, np.where(dw < 0, (ROOM_LO - c) / dw, np.inf))
        r = tt.min(axis=1) + rng.normal(0, noise, rings)
        pts[:, j, :3] = d * r[:, None]
        pts[:, j, 3] = np.arange(rings) + SCAN_PERIOD * rel
    Rs, cs = pose_at(t0); Re, ce = pose_at(t0 + SCAN_PERIOD)
    Rse = Re.T @ Rs; tse = Re.T @ (cs - ce)                                                         # end <- start
    yaw = np.arctan2(Rse[1, 0], Rse[0, 0])
    g = np.eye(4)
    if k > 0:
        Rp, cp = pose_at(t0)                                                                        # the previous scan ended where this one starts
        g[:3, :3] = Rp.T @ Re; g[:3, 3] = Rp.T @ (ce - cp)
    return pts.reshape(-1, 4).astype(np.float32), _f(quat_z(yaw)), _f(tse), g


@functools.lru_cache(maxsize=None)
def chain(n_scans=6, rings=16, az=225):
    return tuple(room_scan(k, rings, az) for k in range(n_scans))


@functools.lru_cache(maxsize=None)
def prefix_scan():
    """One 1025-point scan whose prefixes are the sizes the compaction is tested at, with every eleventh point made to fail a gate;
    (xyzi, q, t, kept cloud 50-digit coordinates by input index, float32 restatement, keep)."""
    xyzi, q, t, _ = room_scan(1, rings=5, az=205, seed=7)
    xyzi = xyzi.copy()
    xyzi[::11, 3] = -xyzi[::11, 3] - 0.5                                                            # s < 0
    xyzi[5::37, 0] = np.nan                                                                         # removed after the transform
    xyzi[7::53, :2] = 0.01                                                                          # inside min_distance
    q, t = MOTIONS["generic"][0], t
    out, keep, _ = deskew_f32(xyzi, q, t)
    return xyzi, q, t, deskew_mp(xyzi, q, t, keep=keep), out, keep
