"""NumPy restatement of include/vilgmap.h (ARITHMETIC CONTRACT steps 1-7), brute force: one operation per NumPy call so that nothing is
fused, every query point against every map point.  Shares no code with the library.  Test infrastructure: O(n_query * n_map) time, meant for
maps of a few ten thousand points.  Also the synthetic room the global-map tests share."""
import numpy as np

F32, F64 = np.float32, np.float64
VOXEL_LIMIT = 1 << 20


def transform(T, xyz):
    """Step 1: points promoted to float64, q_r = ((m_r0 * x + m_r1 * y) + m_r2 * z) + m_r3, rounded to float32.  n x 3 float32."""
    m = np.asarray(T, F64).reshape(4, 4)
    p = np.ascontiguousarray(xyz, F32).reshape(-1, 3).astype(F64)
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    return np.stack([((m[r, 0] * x + m[r, 1] * y) + m[r, 2] * z) + m[r, 3] for r in range(3)], axis=1).astype(F32)


def voxel(p, res, origin=(0.0, 0.0, 0.0)):
    """Step 2: n x 3 int64 voxel indices of float32 points at float32 resolution res.  ValueError outside 2^20."""
    p = np.ascontiguousarray(p, F32).reshape(-1, 3).astype(F64)
    c = np.floor((p - np.asarray(origin, F64)[None, :]) / F64(F32(res))).astype(np.int64)
    if len(c) and np.abs(c).max() >= VOXEL_LIMIT:
        raise ValueError("voxel index outside 2^20")
    return c


def pack(c):
    """The voxel's 63-bit key."""
    c = c + VOXEL_LIMIT
    return (c[:, 0] << 42) | (c[:, 1] << 21) | c[:, 2]


def sqdist(q, m):
    """len(q) x len(m) float32: (dx * dx + dy * dy) + dz * dz."""
    d = q[:, None, :] - m[None, :, :]
    d = d * d
    s = (d[:, :, 0] + d[:, :, 1]) + d[:, :, 2]
    assert s.dtype == F32
    return s


class RefMap:
    """The map as include/vilgmap.h defines it: `points` (n x 3 float32, in insertion order), the stored scans, the voxel keys of the points."""

    def __init__(self, map_resolution=0.05, origin=(0.0, 0.0, 0.0)):
        self.res, self.origin = F32(map_resolution), tuple(float(v) for v in origin)
        self.scans = {}
        self.clear()

    def clear(self):
        self.points = np.zeros((0, 3), F32)
        self.keys = np.zeros(0, np.int64)

    def add_scan(self, key, xyz):
        assert key not in self.scans
        self.scans[key] = np.ascontiguousarray(xyz, F32).reshape(-1, 3).copy()

    def insert_world(self, q):
        """Step 3 for points already in the world.  Returns the survivors' input indices."""
        q = np.ascontiguousarray(q, F32).reshape(-1, 3)
        if not self.res > 0:
            keep = np.arange(len(q))
        else:
            k = pack(voxel(q, self.res, self.origin))
            _, first = np.unique(k, return_index=True)                  # the first input point of every voxel
            first.sort()
            keep = first[~np.isin(k[first], self.keys)]                 # whose voxel holds no map point
            self.keys = np.concatenate([self.keys, k[keep]])
        self.points = np.concatenate([self.points, q[keep]])
        return keep

    def insert(self, xyz, T):
        return self.insert_world(transform(T, xyz))

    def insert_key(self, key, T):
        return self.insert(self.scans[key], T)

    def rebuild(self, keys, Ts):
        """Step 4: one input, the stored scans concatenated in key order."""
        Ts = np.asarray(Ts, F64).reshape(-1, 4, 4)
        q = np.concatenate([transform(T, self.scans[k]) for k, T in zip(keys, Ts)])
        if self.res > 0:
            voxel(q, self.res, self.origin)                             # refused before anything changes
        self.clear()
        return self.insert_world(q)

    def _out(self, idx, T_out):
        idx = np.asarray(idx, np.int32)
        p = self.points[idx]
        return (transform(T_out, p) if T_out is not None else p.copy()), idx

    def in_radius(self, xyz, T, radius, rows=64):
        """Step 5's set U as a bool mask over the map points."""
        q = transform(T, xyz)
        r2 = F32(F64(radius) * F64(radius))
        hit = np.zeros(len(self.points), bool)
        for a in range(0, len(q), rows):
            hit |= (sqdist(q[a:a + rows], self.points) <= r2).any(axis=0)
        return hit

    def reference_radius(self, xyz, T, radius=0.5, ref_resolution=0.3, T_out=None):
        """Steps 5 and 7: (ref_xyz, ref_idx)."""
        u = np.nonzero(self.in_radius(xyz, T, radius))[0]
        if F32(ref_resolution) > 0 and len(u):
            k = pack(voxel(self.points[u], ref_resolution, self.origin))
            _, first = np.unique(k, return_index=True)                  # u ascends: the first of a voxel is its smallest j
            u = u[np.sort(first)]
        return self._out(u, T_out)

    def knn(self, xyz, T, k=5, max_dist=1.5, rows=64):
        """Step 6 per query point: a list of (d2 float32 array, j array), each sorted by (d2, j)."""
        q = transform(T, xyz)
        out = []
        for a in range(0, len(q), rows):
            s = sqdist(q[a:a + rows], self.points)
            for row in s:
                j = np.nonzero(row <= F32(max_dist))[0]
                o = np.lexsort((j, row[j]))[:k]
                out.append((row[j][o], j[o]))
        return out

    def reference_knn(self, xyz, T, k=5, max_dist=1.5, T_out=None):
        """Steps 6 and 7: (ref_xyz, ref_idx), query after query."""
        if not len(self.points):
            return self._out(np.zeros(0, np.int32), T_out)
        return self._out(np.concatenate([j for _, j in self.knn(xyz, T, k, max_dist)] + [np.zeros(0, np.int64)]), T_out)


# ---- the synthetic room: a 12 x 8 x 3 m box seen from 12 sensor poses along a 7.7 m path, 0.2 rad of yaw per pose, 1500 rays each
ROOM = np.array([12.0, 8.0, 3.0])


def pose(x, y, z, yaw):
    c, s = np.cos(yaw), np.sin(yaw)
    T = np.eye(4)
    T[:3, :3] = [[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]]
    T[:3, 3] = [x, y, z]
    return T


def room_poses(n=12):
    return [pose(2.0 + 0.7 * k, 4.0, 1.2, 0.2 * k) for k in range(n)]


def room_scan(T, rays=1500, seed=0):
    """The box's surface seen from pose T (sensor -> world): rays x 3 float32 in the sensor frame."""
    rng = np.random.default_rng(seed)
    d = rng.normal(size=(rays, 3))
    d /= np.linalg.norm(d, axis=1)[:, None]
    dw = d @ T[:3, :3].T
    o = T[:3, 3]
    with np.errstate(divide="ignore"):
        t = np.where(dw > 0, (ROOM - o) / dw, np.where(dw < 0, -o / dw, np.inf)).min(axis=1)
    return (d * t[:, None]).astype(F32)


_ROOM_CACHE = {}


def room(n=12, rays=1500):
    """(poses, scans) of the room, computed once; treat as read-only."""
    if (n, rays) not in _ROOM_CACHE:
        poses = room_poses(n)
        _ROOM_CACHE[(n, rays)] = (poses, [room_scan(T, rays, seed=100 + k) for k, T in enumerate(poses)])
    return _ROOM_CACHE[(n, rays)]
