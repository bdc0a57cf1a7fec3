"""NumPy restatement of the contract of include/villmap.h (lidar_mapping's local cube map), for tests/test_localmap_ref.py and
tests/test_gpu_localmap.py.

  LocalMapRef   a SEQUENTIAL, cube-by-cube transcription of process(): Python lists of arrays, cloud_ref.filter_seq per cube, the six
                while loops as written.
  LocalMapDict  a second, independent formulation: cube keys computed vectorised, the cubes a dict keyed by WORLD cube coordinate (a
                shift moves the window, not the cubes), cloud_ref.filter_part per cube.
  walk / room_chain   the inputs the tests share.
Nothing here is checked against PCL's bits (the header says why).  The alignment is not restated: `align` is a callback (the tests hand
in the library's public vmap_set_map + vmap_align), and without it the pose stays the guess."""
import functools

import numpy as np

import cloud_ref

F = np.float32
W, H, D = 11, 11, 7
CUBES = W * H * D
DIM = (W, H, D)
DEFAULTS = dict(line_res=0.2, plane_res=0.4, hist_size=512, publish_first_frame=10, cube_length=10.0, cube_height=5.0, publish_distance=2.0, publish_frames=30)


def empty():
    return np.zeros((0, 4), F)


def pts(a):
    return np.ascontiguousarray(a, F).reshape(-1, 4)


# ---- step 1 / 5 / 8: the host's double arithmetic, in the header's order ------------------------------------------------------------------
def quat_mul(a, b):
    """Eigen's product, [x y z w]."""
    a = [float(v) for v in a]; b = [float(v) for v in b]
    w = a[3] * b[3] - a[0] * b[0] - a[1] * b[1] - a[2] * b[2]
    x = a[3] * b[0] + a[0] * b[3] + a[1] * b[2] - a[2] * b[1]
    y = a[3] * b[1] + a[1] * b[3] + a[2] * b[0] - a[0] * b[2]
    z = a[3] * b[2] + a[2] * b[3] + a[0] * b[1] - a[1] * b[0]
    return np.array([x, y, z, w])


def quat_rot(q, v):
    """Eigen's quaternion * vector."""
    q = [float(c) for c in q]; v = [float(c) for c in v]
    uv = [q[1] * v[2] - q[2] * v[1], q[2] * v[0] - q[0] * v[2], q[0] * v[1] - q[1] * v[0]]
    uv = [c + c for c in uv]
    c = [q[1] * uv[2] - q[2] * uv[1], q[2] * uv[0] - q[0] * uv[2], q[0] * uv[1] - q[1] * uv[0]]
    return np.array([(v[k] + q[3] * uv[k]) + c[k] for k in range(3)])


def quat_inv(q):
    q = [float(c) for c in q]
    n2 = ((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]) + q[3] * q[3]
    return np.array([-q[0] / n2, -q[1] / n2, -q[2] / n2, q[3] / n2])


def quat_to_R(q):
    """The library's host quat_to_R (vilmap.hip), row-major 3 x 3."""
    x, y, z, w = (float(c) for c in q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


def matrix_of(q, t):
    return np.concatenate([quat_to_R(q), np.asarray(t, np.float64).reshape(3, 1)], axis=1)


# ---- steps 2 / 6: the cube of a coordinate -------------------------------------------------------------------------------------------------
def cube_index(v, size, cen, half=0.0, decrement=True):
    """int((v + H) / size) + cen, minus one when v + H < 0.  half = 0.0 is the QUIRK; the two keyword arguments are the mutants."""
    s = float(v) + half
    c = int(s / size) + cen                                                      # int() truncates toward zero, as the C cast
    if decrement and s < 0:
        c -= 1
    return c


def to_map(M, p):
    """pointAssociateToMap with the 3 x 4 double matrix M: ((r0 x + r1 y) + r2 z) + r3 in double, rounded to float."""
    p = pts(p); M = np.asarray(M, np.float64).reshape(3, 4)
    x, y, z = (p[:, k].astype(np.float64) for k in range(3))
    out = p.copy()
    for r in range(3):
        out[:, r] = (((M[r, 0] * x + M[r, 1] * y) + M[r, 2] * z) + M[r, 3]).astype(F)
    return out


def to_sensor(R, t, p):
    """the /local_map copy: per row c of R^T, ((R0c dx + R1c dy) + R2c dz) with d = p - t in double, rounded to float."""
    p = pts(p)
    d = [p[:, k].astype(np.float64) - float(t[k]) for k in range(3)]
    out = p.copy()
    for c in range(3):
        out[:, c] = ((R[0, c] * d[0] + R[1, c] * d[1]) + R[2, c] * d[2]).astype(F)
    return out


def valid_cubes(ctr):
    out = []
    for i in range(ctr[0] - 2, ctr[0] + 3):
        for j in range(ctr[1] - 2, ctr[1] + 3):
            for k in range(ctr[2] - 1, ctr[2] + 2):
                if 0 <= i < W and 0 <= j < H and 0 <= k < D:
                    out.append(i + W * j + W * H * k)
    return out


class Result:
    """What one push leaves for the tests to compare."""

    def __init__(self, **kw):
        self.__dict__.update(kw)

    def counts(self):
        """as localmap.summary_counts of the device's summary"""
        return (tuple(self.shift), len(self.from_map[0]), len(self.from_map[1]), len(self.stack[0]), len(self.stack[1]), self.aligned, self.n_added[0], self.n_added[1],
                self.n_map[0], self.n_map[1], int(self.published is not None), self.frame_count)


class _State:
    def __init__(self, half_cube=False, decrement=True, **cfg):
        bad = set(cfg) - set(DEFAULTS)
        assert not bad, bad
        self.cfg = {**DEFAULTS, **cfg}
        self.half = (0.5 * self.cfg["cube_length"], 0.5 * self.cfg["cube_length"], 0.5 * self.cfg["cube_height"]) if half_cube else (0.0, 0.0, 0.0)
        self.decrement = decrement
        self.size = (self.cfg["cube_length"], self.cfg["cube_length"], self.cfg["cube_height"])
        self.leaf = (self.cfg["line_res"], self.cfg["plane_res"])
        self.reset()

    def reset(self):
        self.cen = [5, 5, 3]
        self.q_wmap_wodom = np.array([0.0, 0.0, 0.0, 1.0]); self.t_wmap_wodom = np.zeros(3)
        self.frame_count = 0; self.last_frame_count = 0; self.first_odom = True
        self.q_last = np.array([0.0, 0.0, 0.0, 1.0]); self.t_last = np.zeros(3)
        self._clear()

    def guess(self, q_wodom, t_wodom):
        return quat_mul(self.q_wmap_wodom, q_wodom), quat_rot(self.q_wmap_wodom, t_wodom) + self.t_wmap_wodom

    def transform_update(self, q, t, q_wodom, t_wodom):
        self.q_wmap_wodom = quat_mul(q, quat_inv(q_wodom))
        self.t_wmap_wodom = np.asarray(t, np.float64) - quat_rot(self.q_wmap_wodom, t_wodom)

    def decide_publication(self, q, t):
        """step 8's state machine; True: publish"""
        g = self.cfg
        pub = False
        if self.first_odom:
            self.q_last, self.t_last = np.array(q, np.float64), np.array(t, np.float64)
            self.last_frame_count = self.frame_count
            if self.frame_count >= g["publish_first_frame"]:
                self.first_odom = False
                pub = True
        else:
            R = quat_to_R(q)
            d = [float(self.t_last[k]) - float(t[k]) for k in range(3)]
            v = [(R[0, c] * d[0] + R[1, c] * d[1]) + R[2, c] * d[2] for c in range(3)]
            if float(np.sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2])) > g["publish_distance"] or self.frame_count - self.last_frame_count > g["publish_frames"]:
                self.q_last, self.t_last = np.array(q, np.float64), np.array(t, np.float64)
                pub = True
                self.last_frame_count = self.frame_count
        return pub

    def push(self, corner, surf, q_wodom, t_wodom, align=None, matrix=None):
        """One scan.  align(from_map_corner, from_map_surf, stack_corner, stack_surf, q, t, gate) -> (q, t, anything) stands for step 5: it
        is told whether the gate passes and returns the pose unchanged when it does not; matrix (3 x 4) overrides the one step 6 uses (the device's own, from its debug stage)."""
        g = self.cfg
        q, t = self.guess(q_wodom, t_wodom)
        shift, ctr = self.centre_and_shift(t)
        valid = valid_cubes(ctr)
        from_map = [self.concat(cls, valid) for cls in range(2)]
        stack = [cloud_ref.filter_seq(pts(c), self.leaf[cls], g["hist_size"]).out for cls, c in enumerate((corner, surf))]
        gate = len(from_map[0]) > 10 and len(from_map[1]) > 50
        aligned, extra = 0, None
        if align is not None:                                                    # (called without the gate too: the map is set on every scan)
            q, t, extra = align(from_map[0], from_map[1], stack[0], stack[1], q.copy(), t.copy(), gate)
            aligned = int(gate)
        self.transform_update(q, t, q_wodom, t_wodom)
        M = matrix_of(q, t) if matrix is None else np.asarray(matrix, np.float64).reshape(3, 4)
        n_added = [self.add(cls, to_map(M, stack[cls])) for cls in range(2)]
        raw = {(cls, e): self.cube(cls, e).copy() for cls in range(2) for e in valid if len(self.cube(cls, e))}     # what step 7 is given
        self.refilter(valid)
        filtered = {key: self.cube(*key).copy() for key in raw}                  # and what it made of it
        n_map = self.totals()
        published = None
        if self.decide_publication(q, t):
            world = self.take_all()
            published = (world, to_sensor(quat_to_R(q), t, world))
            self.q_wmap_wodom = np.array([0.0, 0.0, 0.0, 1.0]); self.t_wmap_wodom = np.zeros(3)
        self.frame_count += 1
        return Result(q=np.array(q, np.float64), t=np.array(t, np.float64), shift=shift, from_map=from_map, stack=stack, aligned=aligned, extra=extra, matrix=M, n_added=n_added,
                      n_map=n_map, published=published, frame_count=self.frame_count, valid=valid, raw=raw, filtered=filtered)

    def key(self, v, axis):
        return cube_index(v, self.size[axis], self.cen[axis], self.half[axis], self.decrement)


class LocalMapRef(_State):
    """The transcription: two lists of 847 arrays and the loops as the reference writes them."""

    def _clear(self):
        self.cubes = [[empty() for _ in range(CUBES)] for _ in range(2)]

    def centre_and_shift(self, t):
        ci, cj, ck = (self.key(t[a], a) for a in range(3))
        shift = [0, 0, 0]
        A = self.cubes
        while ci < 3:
            for j in range(H):
                for k in range(D):
                    for cls in range(2):
                        for i in range(W - 1, 0, -1):
                            A[cls][i + W * j + W * H * k] = A[cls][i - 1 + W * j + W * H * k]
                        A[cls][0 + W * j + W * H * k] = empty()
            ci += 1; self.cen[0] += 1; shift[0] += 1
        while ci >= W - 3:
            for j in range(H):
                for k in range(D):
                    for cls in range(2):
                        for i in range(0, W - 1):
                            A[cls][i + W * j + W * H * k] = A[cls][i + 1 + W * j + W * H * k]
                        A[cls][W - 1 + W * j + W * H * k] = empty()
            ci -= 1; self.cen[0] -= 1; shift[0] -= 1
        while cj < 3:
            for i in range(W):
                for k in range(D):
                    for cls in range(2):
                        for j in range(H - 1, 0, -1):
                            A[cls][i + W * j + W * H * k] = A[cls][i + W * (j - 1) + W * H * k]
                        A[cls][i + W * 0 + W * H * k] = empty()
            cj += 1; self.cen[1] += 1; shift[1] += 1
        while cj >= H - 3:
            for i in range(W):
                for k in range(D):
                    for cls in range(2):
                        for j in range(0, H - 1):
                            A[cls][i + W * j + W * H * k] = A[cls][i + W * (j + 1) + W * H * k]
                        A[cls][i + W * (H - 1) + W * H * k] = empty()
            cj -= 1; self.cen[1] -= 1; shift[1] -= 1
        while ck < 3:
            for i in range(W):
                for j in range(H):
                    for cls in range(2):
                        for k in range(D - 1, 0, -1):
                            A[cls][i + W * j + W * H * k] = A[cls][i + W * j + W * H * (k - 1)]
                        A[cls][i + W * j + W * H * 0] = empty()
            ck += 1; self.cen[2] += 1; shift[2] += 1
        while ck >= D - 3:
            for i in range(W):
                for j in range(H):
                    for cls in range(2):
                        for k in range(0, D - 1):
                            A[cls][i + W * j + W * H * k] = A[cls][i + W * j + W * H * (k + 1)]
                        A[cls][i + W * j + W * H * (D - 1)] = empty()
            ck -= 1; self.cen[2] -= 1; shift[2] -= 1
        return shift, (ci, cj, ck)

    def concat(self, cls, valid):
        return np.concatenate([self.cubes[cls][e] for e in valid] + [empty()])

    def add(self, cls, placed):
        n = 0
        for p in placed:                                                         # one point at a time, as the reference
            if not (np.isfinite(p[0]) and np.isfinite(p[1]) and np.isfinite(p[2])):
                continue                                                         # the DEVIATION
            i, j, k = (self.key(np.float64(p[a]), a) for a in range(3))
            if 0 <= i < W and 0 <= j < H and 0 <= k < D:
                e = i + W * j + W * H * k
                self.cubes[cls][e] = np.concatenate([self.cubes[cls][e], p[None, :]])
                n += 1
        return n

    def refilter(self, valid):
        for e in valid:
            for cls in range(2):
                self.cubes[cls][e] = cloud_ref.filter_seq(self.cubes[cls][e], self.leaf[cls], self.cfg["hist_size"]).out

    def totals(self):
        return [sum(len(c) for c in self.cubes[cls]) for cls in range(2)]

    def take_all(self):
        parts = []
        for e in range(CUBES):
            parts += [self.cubes[0][e], self.cubes[1][e]]
            self.cubes[0][e] = empty(); self.cubes[1][e] = empty()
        return np.concatenate(parts + [empty()])

    def cube(self, cls, e):
        return self.cubes[cls][e]


class LocalMapDict(_State):
    """The second formulation.  A cube's WORLD coordinate is its array index minus (cenW, cenH, cenD); both move together in a shift, so
    a shift only moves the window [-cen, dim - 1 - cen] and drops what falls out of it."""

    def _clear(self):
        self.world = [{}, {}]

    def keys_of(self, xyz):
        """vectorised cube_index without the centre: n x 3 int64"""
        s = np.asarray(xyz, np.float64) + np.asarray(self.half)
        k = np.trunc(s / np.asarray(self.size)).astype(np.int64)
        if self.decrement:
            k = k - (s < 0)
        return k

    def centre_and_shift(self, t):
        w = self.keys_of(np.asarray(t, np.float64).reshape(1, 3))[0]
        shift = [0, 0, 0]
        for a in range(3):
            c = int(w[a]) + self.cen[a]
            new = self.cen[a] + (3 - c if c < 3 else 0) - (c - (DIM[a] - 4) if c >= DIM[a] - 3 else 0)
            shift[a] = new - self.cen[a]
            self.cen[a] = new
        for cls in range(2):
            self.world[cls] = {k: v for k, v in self.world[cls].items() if all(0 <= k[a] + self.cen[a] < DIM[a] for a in range(3))}
        return shift, tuple(int(w[a]) + self.cen[a] for a in range(3))

    def _index(self, k):
        return (k[0] + self.cen[0]) + W * (k[1] + self.cen[1]) + W * H * (k[2] + self.cen[2])

    def _world_of(self, e):
        return (e % W - self.cen[0], (e // W) % H - self.cen[1], e // (W * H) - self.cen[2])

    def concat(self, cls, valid):
        return np.concatenate([self.world[cls].get(self._world_of(e), empty()) for e in valid] + [empty()])

    def add(self, cls, placed):
        ok = np.isfinite(placed[:, :3]).all(axis=1)
        k = self.keys_of(np.where(ok[:, None], placed[:, :3], 0.0))
        ok &= ((k + np.asarray(self.cen) >= 0) & (k + np.asarray(self.cen) < np.asarray(DIM))).all(axis=1)
        kept, kk = placed[ok], k[ok]
        for key in sorted(set(map(tuple, kk.tolist()))):
            sel = (kk == np.asarray(key)).all(axis=1)
            self.world[cls][key] = np.concatenate([self.world[cls].get(key, empty()), kept[sel]])
        return int(ok.sum())

    def refilter(self, valid):
        for cls in range(2):
            for e in valid:
                k = self._world_of(e)
                if k in self.world[cls]:
                    self.world[cls][k] = pts(cloud_ref.filter_part(self.world[cls][k], self.leaf[cls], self.cfg["hist_size"]))

    def totals(self):
        return [sum(len(c) for c in self.world[cls].values()) for cls in range(2)]

    def take_all(self):
        order = sorted(set(self.world[0]) | set(self.world[1]), key=self._index)
        parts = []
        for k in order:
            parts += [self.world[0].get(k, empty()), self.world[1].get(k, empty())]
        self.world = [{}, {}]
        return np.concatenate(parts + [empty()])

    def cube(self, cls, e):
        return self.world[cls].get(self._world_of(e), empty())


def state_bytes(m, res):
    """Everything a push leaves, as bytes: what the two formulations and the device are compared on."""
    parts = [np.asarray(res.counts()[0], np.int64).tobytes(), np.asarray(res.counts()[1:], np.int64).tobytes(), res.q.tobytes(), res.t.tobytes()]
    parts += [c.tobytes() for c in res.from_map + res.stack]
    if res.published is not None:
        parts += [res.published[0].tobytes(), res.published[1].tobytes()]
    for cls in range(2):
        for e in range(CUBES):
            c = m.cube(cls, e)
            if len(c):
                parts += [np.asarray([cls, e, len(c)], np.int64).tobytes(), c.tobytes()]
    return b"".join(parts)


# ---- shared inputs ------------------------------------------------------------------------------------------------------------------------
def yaw_quat(a):
    return np.array([0.0, 0.0, np.sin(0.5 * a), np.cos(0.5 * a)])


def walk(seed=0, n=30, n_corner=40, n_surf=160):
    """A random walk that leaves the array in both directions, with scans that reach several cubes: [(corner, surf, q, t)]."""
    rng = np.random.default_rng(seed)
    t = np.array([1.0, -2.0, 0.5]); out = []
    for k in range(n):
        step = rng.uniform(-9.0, 9.0, 3) * np.array([1.0, 1.0, 0.4])
        if k % 7 == 6:
            step *= 4.0                                                          # a jump of several cubes
        t = t + step
        q = yaw_quat(rng.uniform(-3.0, 3.0))
        clouds = []
        for m in (n_corner, n_surf):
            xyz = rng.uniform(-1.0, 1.0, (m, 3)) * np.array([28.0, 28.0, 9.0])
            xyz[: m // 4] = np.round(xyz[: m // 4] / 5.0) * 5.0 - t              # coordinates that land on cube boundaries once translated (yaw aside)
            clouds.append(np.concatenate([xyz, rng.uniform(0.0, 50.0, (m, 1))], axis=1).astype(F))
        out.append((clouds[0], clouds[1], q, t.copy()))
    return out


@functools.lru_cache(maxsize=None)
def room_chain(n=10):
    """A walk through mapreg's room across the cube boundary x = 0: [(corner, surf, q_wodom, t_wodom)], a few hundred corner and a couple of
    thousand surf points per scan; the odometry drifts a little, so the alignment has something to do."""
    from mvil_fusion_amd import mapreg
    cmap, smap = mapreg.make_map(seed=3, n_surf=9000, n_corner=1500)
    out = []
    for k in range(n):
        a = 0.2 + 0.05 * k
        Rk = np.array([[np.cos(a), -np.sin(a), 0.0], [np.sin(a), np.cos(a), 0.0], [0.0, 0.0, 1.0]])
        tk = np.array([-1.3 + 0.45 * k, 0.6 - 0.1 * k, 0.2])
        corner, surf = mapreg.make_scan(cmap, smap, Rk, tk, seed=70 + k, n_surf=2000, n_corner=300)
        q = yaw_quat(a + 0.002 * k)
        out.append((pts(corner), pts(surf), q, tk + np.array([0.01 * k, -0.008 * k, 0.002 * k])))
    return out
