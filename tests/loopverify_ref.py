"""NumPy restatement of vloop_score and of vloop_verify's selection rule (include/villoop.h, ARITHMETIC CONTRACT steps 1-5), brute force:
every source point against every target point in float32, one operation per NumPy call so that nothing is fused.  Test infrastructure:
O(n_source * n_target) memory and time, meant for clouds of a few thousand points."""
import sys

import numpy as np

F32 = np.float32
DBL_MAX = sys.float_info.max
SUM_BLOCK = 256


def round_transform(T):
    """Step 1: the first three rows of T as float32 (3 x 4)."""
    return np.asarray(T, np.float64).reshape(4, 4)[:3].astype(F32)


def transform(T, src):
    """Step 2: q_r = ((m_r0 * x + m_r1 * y) + m_r2 * z) + m_r3 in float32.  Returns n x 3 float32."""
    m = round_transform(T)
    src = np.ascontiguousarray(src, F32).reshape(-1, 3)
    x, y, z = src[:, 0], src[:, 1], src[:, 2]
    return np.stack([((m[r, 0] * x + m[r, 1] * y) + m[r, 2] * z) + m[r, 3] for r in range(3)], axis=1).astype(F32)


def nearest(q, tgt, rows=512):
    """Step 3 for transformed points q: (d2 float32, idx int32) per point; d2 = (dx * dx + dy * dy) + dz * dz in float32, the minimum over all
    target points, the smallest index among equal distances (argmin returns the first)."""
    q = np.ascontiguousarray(q, F32).reshape(-1, 3); tgt = np.ascontiguousarray(tgt, F32).reshape(-1, 3)
    d2 = np.empty(len(q), F32); idx = np.empty(len(q), np.int32)
    for a in range(0, len(q), rows):
        d = q[a:a + rows, None, :] - tgt[None, :, :]
        d = d * d
        s = (d[:, :, 0] + d[:, :, 1]) + d[:, :, 2]
        assert s.dtype == F32
        j = np.argmin(s, axis=1)
        idx[a:a + rows] = j; d2[a:a + rows] = s[np.arange(len(j)), j]
    return d2, idx


def block_total(d2, max_range=DBL_MAX):
    """Steps 4 and 5 before the division: (sum float64, n_used).  Sequential sums in ascending order inside blocks of 256 consecutive
    points, then over the block partials in ascending order; a point is used when float64(d2) <= max_range."""
    d = np.asarray(d2, F32).astype(np.float64)
    used = d <= max_range
    total, n_used = 0.0, 0
    for b in range(0, len(d), SUM_BLOCK):
        part = 0.0
        for v, u in zip(d[b:b + SUM_BLOCK].tolist(), used[b:b + SUM_BLOCK].tolist()):
            if u:
                part = part + v; n_used += 1
        total = total + part
    return total, n_used


def block_sum(d2, max_range=DBL_MAX):
    """(score float64, n_used): the sum over n_used, DBL_MAX when nothing is used."""
    total, n_used = block_total(d2, max_range)
    return (total / n_used if n_used else DBL_MAX), n_used


def score(T, src, tgt, max_range=DBL_MAX):
    """vloop_score for one transform: (score, n_used, nn_d2, nn_idx)."""
    d2, idx = nearest(transform(T, src), tgt)
    s, n = block_sum(d2, max_range)
    return s, n, d2, idx


def select(fitness, converged, max_tolerable_fitness):
    """vloop_verify's selection: the first candidate whose float32 fitness is strictly below the running minimum, which starts at
    max_tolerable_fitness; a candidate that did not converge is skipped.  Returns (index or -1, the running minimum)."""
    run, best = F32(max_tolerable_fitness), -1
    for k, (f, c) in enumerate(zip(fitness, converged)):
        if c and F32(f) < run:
            run, best = F32(f), k
    return best, run


def inverse_isometry(T):
    """(R, t) -> (R^-1, -R^-1 t) in float64: the inverse of a float-rounded isometry, whose R is orthonormal to 6e-8 only."""
    T = np.asarray(T, np.float64).reshape(4, 4)
    D = np.eye(4)
    D[:3, :3] = np.linalg.inv(T[:3, :3])
    D[:3, 3] = -(D[:3, :3] @ T[:3, 3])
    return D
