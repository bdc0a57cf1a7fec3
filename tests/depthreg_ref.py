"""numpy float32 restatement of DepthRegister::get_depth (feature_tracker_/src/feature_tracker.h:98-343) as include/vildepth.h states it,
steps 1-9.  Every operation is one float32 numpy operation in the header's order (numpy does not fuse a * b + c); the marked places are
float64.  The 3-NN is a brute-force search over ALL sphere points: it shares neither the row band nor any code with the kernels."""
import math

import numpy as np

BINS = 360
MIN_SPHERE = 10
F = np.float32
THRESHOLD = F(math.pow(math.sin(0.5 / 180.0 * math.pi) * 5.0, 2))           # :268, evaluated in double
FLT_MAX = np.finfo(np.float32).max


class Result:
    """depth (n_feat), nn3 (n_feat x 3), sphere (n_sphere x 4), sphere_rc (row, col per sphere point), sphere_src (cloud index per sphere
    point), n_cloud / n_in_view / n_sphere / n_with_depth."""


def roundf(v):
    """C's roundf on a float32 array: halves away from zero (np.round goes to even)."""
    a = np.abs(v)
    r = np.floor(a)
    r = r + ((a - r) >= F(0.5)).astype(np.float32)                           # a - floor(a) is exact
    return np.copysign(r, v)


def apply34(m, x, y, z):
    m = np.asarray(m, np.float32).reshape(3, 4)
    return tuple(((m[r, 0] * x + m[r, 1] * y) + m[r, 2] * z) + m[r, 3] for r in range(3))


def angles(x, y, z):
    """step 3: row_angle, col_angle (float32) of float32 arrays."""
    with np.errstate(all="ignore"):
        ele = np.arctan2(z, np.sqrt(x * x + y * y))
        row_angle = (ele.astype(np.float64) * 180.0 / math.pi + 90.0).astype(np.float32)
        col_angle = (np.arctan2(x, y).astype(np.float64) * 180.0 / math.pi).astype(np.float32)
    return row_angle, col_angle


def bins(x, y, z):
    ra, ca = angles(x, y, z)
    with np.errstate(all="ignore"):
        return roundf(ra / F(0.5)).astype(np.int64), roundf(ca / F(0.5)).astype(np.int64)


def view(cloud, m1, m2):
    """steps 1-2: the transformed points (float32 x, y, z) and the mask of the points that are finite and in view."""
    c = np.ascontiguousarray(cloud, np.float32).reshape(-1, 4)
    with np.errstate(all="ignore"):
        ax, ay, az = apply34(m1, c[:, 0], c[:, 1], c[:, 2])
        ok = np.isfinite(ax) & np.isfinite(ay) & np.isfinite(az)
        x, y, z = apply34(m2, ax, ay, az)
        ok &= np.isfinite(x) & np.isfinite(y) & np.isfinite(z)
        skip = (x < 0) | (np.abs(y / x) > F(10)) | (np.abs(z / x) > F(10))
    return x, y, z, ok & ~skip


def edge_distance(cloud, m1, m2):
    """Per cloud point: how far row_angle * 2 and col_angle * 2 are from the nearest half-integer (the bin edges), in bins; inf for a point
    that steps 1-2 drop.  The GPU tests keep the points whose distance is >= 1e-3 (an input choice, test_gpu_depthreg.py)."""
    x, y, z, ok = view(cloud, m1, m2)
    ra, ca = angles(x, y, z)
    d = np.full(len(x), np.inf)
    for a in (ra, ca):
        v = a.astype(np.float64) * 2.0
        d = np.minimum(d, np.abs(v - np.floor(v) - 0.5))
    d[~ok] = np.inf
    return d


def register(cloud, m1, m2, feat):
    cloud = np.ascontiguousarray(cloud, np.float32).reshape(-1, 4)
    feat = np.ascontiguousarray(feat, np.float32).reshape(-1, 3)
    out = Result()
    nf = len(feat)
    out.depth = np.full(nf, -1.0, np.float32); out.nn3 = np.full((nf, 3), -1, np.int32)
    out.sphere = np.zeros((0, 4), np.float32); out.sphere_rc = np.zeros((0, 2), np.int64); out.sphere_src = np.zeros(0, np.int64)
    out.n_cloud = len(cloud); out.n_in_view = out.n_sphere = out.n_with_depth = 0
    if len(cloud) == 0:
        return out
    x, y, z, ok = view(cloud, m1, m2)
    row, col = bins(x, y, z)
    with np.errstate(all="ignore"):
        dist = np.sqrt(x * x + y * y + z * z)
    ok &= (row >= 0) & (row < BINS) & (col >= 0) & (col < BINS) & (dist > 0) & (dist < FLT_MAX)
    idx = np.nonzero(ok)[0]
    out.n_in_view = len(idx)
    # step 4: strict <, so the first of equal distances stays; step 5: row-major emission
    order = idx[np.lexsort((idx, dist[idx], row[idx] * BINS + col[idx]))]
    b = row[order] * BINS + col[order]
    first = np.ones(len(order), bool); first[1:] = b[1:] != b[:-1]
    win = order[first]
    rng = dist[win]
    out.sphere = np.stack([x[win] / rng, y[win] / rng, z[win] / rng, rng], axis=1).astype(np.float32)      # step 6
    out.sphere_rc = np.stack([row[win], col[win]], axis=1); out.sphere_src = win
    out.n_sphere = len(win)
    if out.n_sphere < MIN_SPHERE or nf == 0:
        return out
    with np.errstate(all="ignore"):
        n = np.sqrt((feat[:, 0] * feat[:, 0] + feat[:, 1] * feat[:, 1]) + feat[:, 2] * feat[:, 2])         # step 7
        v = feat / n[:, None]
    p = np.stack([v[:, 2], -v[:, 0], -v[:, 1]], axis=1)
    s = out.sphere
    for i in range(nf):
        if not np.all(np.isfinite(p[i])):
            continue
        dx, dy, dz = p[i, 0] - s[:, 0], p[i, 1] - s[:, 1], p[i, 2] - s[:, 2]
        d2 = (dx * dx + dy * dy) + dz * dz                                                                  # step 8
        nn = np.argsort(d2, kind="stable")[:3]                                                              # (distance, index)
        if len(nn) < 3 or not d2[nn[2]] < THRESHOLD:
            continue
        out.nn3[i] = nn
        r1, r2, r3 = s[nn[0], 3], s[nn[1], 3], s[nn[2], 3]                                                  # step 9
        if max(r1, r2, r3) - min(r1, r2, r3) > F(2):
            continue
        mean = ((r1 + r2) + r3) / F(3)
        d = p[i, 0] * mean
        if d > F(3.0):
            out.depth[i] = d
    out.n_with_depth = int((out.depth != -1).sum())
    return out


def feature_rows(feat):
    """Range-image row of each feature's sphere point (step 3's formula), for the band tests."""
    feat = np.ascontiguousarray(feat, np.float32).reshape(-1, 3)
    n = np.sqrt((feat[:, 0] * feat[:, 0] + feat[:, 1] * feat[:, 1]) + feat[:, 2] * feat[:, 2])
    v = feat / n[:, None]
    return bins(v[:, 2], -v[:, 0], -v[:, 1])[0]
