"""CPU restatement of include/vilepi.h: a transcription of that header's numbered contract and of nothing else (no OpenCV, no camodocal).
Every float operation is an unfused IEEE operation in the order the header writes it; NumPy does the elementwise ones (it never contracts
a * b + c), Python floats the rest.  The Jacobi of step 4 runs for a whole block of hypotheses at once: the same rotation order, each
hypothesis' own skip, so the arithmetic per hypothesis is that of the serial loop."""
import math

import numpy as np

F32, F64 = np.float32, np.float64
M64 = (1 << 64) - 1
SAMPLE, SWEEPS, LIFT_STEPS = 8, 10, 8                     # VEPI_SAMPLE, VEPI_JACOBI_SWEEPS, VEPI_LIFT_STEPS
MAX_DRAWS = 65536                                         # step 3 gives up after this many draws
HYP_MUL, MIX_ADD, MIX_M1, MIX_M2 = 0xD1342543DE82EF95, 0x9E3779B97F4A7C15, 0xBF58476D1CE4E5B9, 0x94D049BB133111EB
DBL_MIN = 2.2250738585072014e-308
REFERENCE_CAMERA = dict(fx=356.37000498, fy=354.92225534, cx=326.87903275, cy=250.93806883, k1=-0.29326213, k2=0.07505211, p1=0.0002761, p2=-0.00026777)


class Camera:
    """step 1: the PINHOLE model and the virtual camera of rejectWithF"""

    def __init__(self, fx, fy, cx, cy, k1=0.0, k2=0.0, p1=0.0, p2=0.0, focal=460.0, width=640, height=480):
        self.fx, self.fy, self.cx, self.cy, self.k1, self.k2, self.p1, self.p2 = (float(v) for v in (fx, fy, cx, cy, k1, k2, p1, p2))
        self.focal, self.width, self.height = float(focal), int(width), int(height)
        self.inv_K11 = 1.0 / self.fx; self.inv_K13 = -self.cx / self.fx
        self.inv_K22 = 1.0 / self.fy; self.inv_K23 = -self.cy / self.fy
        self.no_distortion = self.k1 == 0.0 and self.k2 == 0.0 and self.p1 == 0.0 and self.p2 == 0.0

    def distortion(self, x, y):
        mx2 = x * x; my2 = y * y; mxy = x * y
        rho2 = mx2 + my2
        rad = self.k1 * rho2 + self.k2 * rho2 * rho2
        return (x * rad + 2.0 * self.p1 * mxy + self.p2 * (rho2 + 2.0 * mx2), y * rad + 2.0 * self.p2 * mxy + self.p1 * (rho2 + 2.0 * my2))

    def lift(self, uv):
        """uv: n x 2 (float32 pixels are widened first).  Returns m_u, n x 2 float64."""
        uv = np.asarray(uv, F64).reshape(-1, 2)
        xd = self.inv_K11 * uv[:, 0] + self.inv_K13
        yd = self.inv_K22 * uv[:, 1] + self.inv_K23
        if self.no_distortion:
            return np.stack([xd, yd], axis=1)
        dx, dy = self.distortion(xd, yd)
        xu = xd - dx; yu = yd - dy
        for _ in range(LIFT_STEPS - 1):
            dx, dy = self.distortion(xu, yu)
            xu = xd - dx; yu = yd - dy
        return np.stack([xu, yu], axis=1)

    def space_to_plane(self, m):
        """PinholeCamera::spaceToPlane of (x, y, 1): only the tests' round trip uses it"""
        m = np.asarray(m, F64).reshape(-1, 2)
        x, y = m[:, 0], m[:, 1]
        if not self.no_distortion:
            dx, dy = self.distortion(x, y)
            x = x + dx; y = y + dy
        return np.stack([self.fx * x + self.cx, self.fy * y + self.cy], axis=1)

    def virtual(self, uv):
        """step 2: float32 points of the virtual camera"""
        m = self.lift(uv)
        return np.stack([self.focal * m[:, 0] + self.width / 2.0, self.focal * m[:, 1] + self.height / 2.0], axis=1).astype(F32)


# ---- step 3 --------------------------------------------------------------------------------------------------------------------------
def mix64(x):
    z = (x + MIX_ADD) & M64
    z = ((z ^ (z >> 30)) * MIX_M1) & M64
    z = ((z ^ (z >> 27)) * MIX_M2) & M64
    return z ^ (z >> 31)


def draw(seed, h, n, max_draws=MAX_DRAWS):
    """(the 8 indices, ok).  ok is False when max_draws draws did not give 8 distinct ones: the rest is 0 and the hypothesis has no model."""
    base = ((seed & M64) ^ ((h * HYP_MUL) & M64)) & M64
    idx, k = [], 0
    while len(idx) < SAMPLE and k < max_draws:
        r = mix64((base + k) & M64); k += 1
        i = ((r >> 32) * n) >> 32
        if i not in idx:
            idx.append(i)
    ok = len(idx) == SAMPLE
    return idx + [0] * (SAMPLE - len(idx)), ok


def sample(seed, h, n):
    return draw(seed, h, n)[0]


# ---- step 4 --------------------------------------------------------------------------------------------------------------------------
def jacobi(A):
    """A: B x N x N symmetric, changed in place.  Returns V (B x N x N, eigenvectors in columns); the eigenvalues are A's diagonal."""
    B, N = A.shape[0], A.shape[1]
    V = np.zeros_like(A); V[:, np.arange(N), np.arange(N)] = 1.0
    with np.errstate(all="ignore"):
        for _ in range(SWEEPS):
            for p in range(N - 1):
                for q in range(p + 1, N):
                    apq = A[:, p, q].copy(); app = A[:, p, p].copy(); aqq = A[:, q, q].copy()
                    on = apq != 0.0
                    if not on.any():
                        continue
                    theta = (aqq - app) / (2.0 * apq)
                    t = np.where(theta >= 0.0, 1.0, -1.0) / (np.abs(theta) + np.sqrt(theta * theta + 1.0))
                    c = 1.0 / np.sqrt(t * t + 1.0)
                    s = t * c
                    for k in range(N):
                        if k != p and k != q:
                            akp = A[:, k, p].copy(); akq = A[:, k, q].copy()
                            np_ = np.where(on, c * akp - s * akq, akp); nq = np.where(on, s * akp + c * akq, akq)
                            A[:, k, p] = np_; A[:, p, k] = np_; A[:, k, q] = nq; A[:, q, k] = nq
                    A[:, p, p] = np.where(on, app - t * apq, app); A[:, q, q] = np.where(on, aqq + t * apq, aqq)
                    z = np.where(on, 0.0, apq); A[:, p, q] = z; A[:, q, p] = z
                    for k in range(N):
                        vkp = V[:, k, p].copy(); vkq = V[:, k, q].copy()
                        V[:, k, p] = np.where(on, c * vkp - s * vkq, vkp); V[:, k, q] = np.where(on, s * vkp + c * vkq, vkq)
    return V


def smallest(A, V):
    """the column of V at the smallest diagonal entry of A, the lowest index among equal ones (as a strict < scan finds it)"""
    B, N = A.shape[0], A.shape[1]
    best = np.zeros(B, np.int64); val = A[:, 0, 0].copy()
    for k in range(1, N):
        lt = A[:, k, k] < val
        best = np.where(lt, k, best); val = np.where(lt, A[:, k, k], val)
    return V[np.arange(B), :, best]


def normalisation(x, y):
    """x, y: B x 8 in sample order.  Returns (cx, cy, scale, ok)."""
    sx = x[:, 0].copy(); sy = y[:, 0].copy()
    for r in range(1, SAMPLE):
        sx = sx + x[:, r]; sy = sy + y[:, r]
    cx = sx / 8.0; cy = sy / 8.0
    d = None
    for r in range(SAMPLE):
        dx = x[:, r] - cx; dy = y[:, r] - cy
        e = np.sqrt(dx * dx + dy * dy)
        d = e if d is None else d + e
    mean = d / 8.0
    ok = mean > 0.0
    with np.errstate(all="ignore"):
        return cx, cy, math.sqrt(2.0) / mean, ok


def fit(p1, p2, idx):
    """idx: B x 8.  Returns (F B x 3 x 3, ok B)."""
    idx = np.asarray(idx, np.int64)
    B = len(idx)
    x1 = p1[idx, 0].astype(F64); y1 = p1[idx, 1].astype(F64); x2 = p2[idx, 0].astype(F64); y2 = p2[idx, 1].astype(F64)
    with np.errstate(all="ignore"):
        c1x, c1y, s1, ok1 = normalisation(x1, y1)
        c2x, c2y, s2, ok2 = normalisation(x2, y2)
        u1 = (x1 - c1x[:, None]) * s1[:, None]; v1 = (y1 - c1y[:, None]) * s1[:, None]
        u2 = (x2 - c2x[:, None]) * s2[:, None]; v2 = (y2 - c2y[:, None]) * s2[:, None]
        R = np.stack([u2 * u1, u2 * v1, u2, v2 * u1, v2 * v1, v2, u1, v1, np.ones_like(u1)], axis=2)          # B x 8 x 9
        A = np.zeros((B, 9, 9))
        for i in range(9):
            for j in range(9):
                acc = R[:, 0, i] * R[:, 0, j]
                for r in range(1, SAMPLE):
                    acc = acc + R[:, r, i] * R[:, r, j]
                A[:, i, j] = acc
        V = jacobi(A)
        Fn = smallest(A, V).reshape(B, 3, 3)
        M = np.zeros((B, 3, 3))
        for i in range(3):
            for j in range(3):
                M[:, i, j] = (Fn[:, 0, i] * Fn[:, 0, j] + Fn[:, 1, i] * Fn[:, 1, j]) + Fn[:, 2, i] * Fn[:, 2, j]
        W = jacobi(M)
        v = smallest(M, W)                                                                                    # B x 3
        Fv = (Fn[:, :, 0] * v[:, None, 0] + Fn[:, :, 1] * v[:, None, 1]) + Fn[:, :, 2] * v[:, None, 2]        # B x 3
        Fn = Fn - Fv[:, :, None] * v[:, None, :]
        t1x = -(s1 * c1x); t1y = -(s1 * c1y); t2x = -(s2 * c2x); t2y = -(s2 * c2y)
        G = np.stack([Fn[:, :, 0] * s1[:, None], Fn[:, :, 1] * s1[:, None], (Fn[:, :, 0] * t1x[:, None] + Fn[:, :, 1] * t1y[:, None]) + Fn[:, :, 2]], axis=2)
        F = np.stack([G[:, 0, :] * s2[:, None], G[:, 1, :] * s2[:, None], (G[:, 0, :] * t2x[:, None] + G[:, 1, :] * t2y[:, None]) + G[:, 2, :]], axis=1)
    ok = ok1 & ok2 & np.isfinite(F).all(axis=(1, 2))
    return F, ok


# ---- step 5 --------------------------------------------------------------------------------------------------------------------------
def errors(F, p1, p2):
    """F 3 x 3; returns (e1, e2): the squared distances of p1 to its line in image 1 and of p2 to its line in image 2"""
    x1 = p1[:, 0].astype(F64); y1 = p1[:, 1].astype(F64); x2 = p2[:, 0].astype(F64); y2 = p2[:, 1].astype(F64)
    f = [float(v) for v in F.reshape(9)]
    with np.errstate(all="ignore"):
        a = (f[0] * x1 + f[1] * y1) + f[2]; b = (f[3] * x1 + f[4] * y1) + f[5]; c = (f[6] * x1 + f[7] * y1) + f[8]
        s2 = 1.0 / (a * a + b * b); d2 = (x2 * a + y2 * b) + c
        e2 = (d2 * d2) * s2
        a = (f[0] * x2 + f[3] * y2) + f[6]; b = (f[1] * x2 + f[4] * y2) + f[7]; c = (f[2] * x2 + f[5] * y2) + f[8]
        s1 = 1.0 / (a * a + b * b); d1 = (x1 * a + y1 * b) + c
        e1 = (d1 * d1) * s1
    return e1, e2


def score(F, p1, p2, thr):
    """(inlier mask, margin): margin = min over the points of |err / thr^2 - 1|, NaN never the minimum (inf without a finite one)"""
    t2 = float(thr) * float(thr)
    e1, e2 = errors(F, p1, p2)
    with np.errstate(all="ignore"):
        inl = (e1 <= t2) & (e2 <= t2)
        err = np.where(e1 > e2, e1, e2)
        m = np.abs(err / t2 - 1.0)
    m = m[~np.isnan(m)]
    return inl, (float(m.min()) if len(m) else math.inf)


# ---- step 6 --------------------------------------------------------------------------------------------------------------------------
def update_iters(confidence, outlier_ratio, max_iters):
    """N of step 6"""
    denom = 1.0 - math.pow(1.0 - outlier_ratio, SAMPLE)
    if denom < DBL_MIN:
        return 0
    num = math.log(1.0 - confidence); denom = math.log(denom)
    if denom >= 0.0 or -num >= max_iters * -denom:
        return max_iters
    return int(round(num / denom))


class Loop:
    """the sequential loop: feed(count) per hypothesis in order while not done"""

    def __init__(self, n, confidence, max_iters):
        self.n, self.confidence, self.max_iters = n, confidence, max_iters
        self.niters, self.h, self.best, self.best_h = max_iters, 0, 0, -1

    @property
    def done(self):
        return self.h >= self.niters

    def feed(self, count):
        if count > max(self.best, SAMPLE - 1):
            self.best, self.best_h = count, self.h
            self.niters = min(self.niters, update_iters(self.confidence, (self.n - count) / self.n, self.max_iters))
        self.h += 1


class Result:
    pass


def reject(cam, cur_xy, forw_xy, thr=1.0, confidence=0.99, seed=1, max_iters=1000, block=64):
    """vepi_reject.  Returns a Result: status (n uint8), found, best_hypothesis, n_inliers, consumed, F (3 x 3 or None), samples (consumed x 8),
    counts (consumed), margins (consumed), margin (their minimum), p1 / p2 (the virtual-camera points)."""
    cur_xy = np.asarray(cur_xy, F32).reshape(-1, 2); forw_xy = np.asarray(forw_xy, F32).reshape(-1, 2)
    n = len(cur_xy)
    r = Result()
    r.status = np.ones(n, np.uint8); r.found, r.best_hypothesis, r.n_inliers, r.consumed, r.F = 0, -1, 0, 0, None
    r.samples = np.zeros((0, SAMPLE), np.int32); r.counts = np.zeros(0, np.int32); r.margins = np.zeros(0); r.margin = math.inf
    r.p1 = r.p2 = np.zeros((0, 2), F32)
    if n < SAMPLE:
        return r
    p1, p2 = cam.virtual(cur_xy), cam.virtual(forw_xy)
    r.p1, r.p2 = p1, p2
    loop = Loop(n, confidence, max_iters)
    samples, counts, margins, best_inl, best_F = [], [], [], None, None
    while not loop.done:
        hs = range(loop.h, min(loop.h + block, loop.niters))
        drawn = [draw(seed, h, n) for h in hs]
        idx = [d[0] for d in drawn]
        Fs, oks = fit(p1, p2, idx)
        oks = oks & np.array([d[1] for d in drawn])
        for k, h in enumerate(hs):
            if loop.done:
                break
            if oks[k]:
                inl, m = score(Fs[k], p1, p2, thr)
            else:
                inl, m = np.zeros(n, bool), math.inf
            cnt = int(inl.sum())
            samples.append(idx[k]); counts.append(cnt); margins.append(m)
            before = loop.best_h
            loop.feed(cnt)
            if loop.best_h != before:
                best_inl, best_F = inl, Fs[k].copy()
    r.samples = np.array(samples, np.int32).reshape(-1, SAMPLE); r.counts = np.array(counts, np.int32); r.margins = np.array(margins, F64)
    r.margin = float(r.margins.min()) if len(margins) else math.inf
    r.consumed = loop.h
    if loop.best_h >= 0:
        r.found, r.best_hypothesis, r.n_inliers, r.F = 1, loop.best_h, loop.best, best_F
        r.status = best_inl.astype(np.uint8)
    return r


# ---- vepi_undistort --------------------------------------------------------------------------------------------------------------------
class Undistorter:
    def __init__(self, cam):
        self.cam = cam
        self.reset()

    def reset(self):
        self.ids, self.un = np.zeros(0, np.int32), np.zeros((0, 2), F32)

    def undistort(self, xy, ids, dt):
        xy = np.asarray(xy, F32).reshape(-1, 2); ids = np.asarray(ids, np.int32).reshape(-1)
        un = self.cam.lift(xy).astype(F32)
        vel = np.zeros((len(xy), 2), F32)
        first = {}
        for j, pid in enumerate(self.ids.tolist()):
            first.setdefault(pid, j)
        with np.errstate(all="ignore"):
            for i, pid in enumerate(ids.tolist()):
                j = first.get(pid, -1) if pid != -1 else -1
                if j >= 0:
                    vel[i] = ((un[i].astype(F64) - self.un[j].astype(F64)) / F64(dt)).astype(F32)
        self.ids, self.un = ids.copy(), un.copy()
        return un, vel


# ---- the two-view scene of the tests ---------------------------------------------------------------------------------------------------
VIRTUAL = dict(fx=460.0, fy=460.0, cx=320.0, cy=240.0)     # lifting through this camera is the identity up to rounding: scenes are built in virtual pixels


def rodrigues(w):
    w = np.asarray(w, F64); th = np.linalg.norm(w)
    K = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]]) / th
    return np.eye(3) + math.sin(th) * K + (1 - math.cos(th)) * (K @ K)


def scene(n, n_out, noise=0.0, seed=0, rvec=(0.02, -0.03, 0.015), tvec=(0.15, 0.02, 0.05)):
    """n correspondences in the 460 / 640 x 480 camera, the LAST n_out of them (after a seeded shuffle: anywhere) moved 8 - 25 px perpendicular
    to their true epipolar line in the second image.  Returns (cur n x 2 float32, forw n x 2 float32, labels n uint8 with 1 = inlier, F_true)."""
    rng = np.random.default_rng(1000 * n + 10 * n_out + seed)
    f, cx, cy = 460.0, 320.0, 240.0
    R, t = rodrigues(rvec), np.asarray(tvec, F64)
    x1 = np.stack([rng.uniform(40, 600, n), rng.uniform(40, 440, n)], axis=1)
    z = rng.uniform(3.0, 12.0, n)
    P = np.stack([(x1[:, 0] - cx) / f * z, (x1[:, 1] - cy) / f * z, z], axis=1)
    Q = P @ R.T + t
    x2 = np.stack([f * Q[:, 0] / Q[:, 2] + cx, f * Q[:, 1] / Q[:, 2] + cy], axis=1)
    Kinv = np.array([[1 / f, 0, -cx / f], [0, 1 / f, -cy / f], [0, 0, 1]])
    tx = np.array([[0, -t[2], t[1]], [t[2], 0, -t[0]], [-t[1], t[0], 0]])
    Ft = Kinv.T @ tx @ R @ Kinv
    labels = np.ones(n, np.uint8)
    out = rng.permutation(n)[:n_out]
    labels[out] = 0
    line = np.concatenate([x1[out], np.ones((n_out, 1))], axis=1) @ Ft.T
    nrm = line[:, :2] / np.linalg.norm(line[:, :2], axis=1, keepdims=True)
    x2[out] += nrm * (rng.uniform(8.0, 25.0, n_out) * rng.choice([-1.0, 1.0], n_out))[:, None]
    if noise:
        x1 = x1 + rng.normal(0.0, noise, x1.shape); x2 = x2 + rng.normal(0.0, noise, x2.shape)
    return x1.astype(F32), x2.astype(F32), labels, Ft


def unit_F(F):
    """unit Frobenius norm, the entry of largest magnitude positive"""
    F = np.asarray(F, F64) / np.linalg.norm(F)
    return F if F.reshape(9)[np.argmax(np.abs(F.reshape(9)))] > 0 else -F
