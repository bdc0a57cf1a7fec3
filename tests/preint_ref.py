"""IMU pre-integration (include/vilpreint.h) restated from the header's contract, in any NumPy precision, plus the instrument
that holds a device record to it.

  preintegrate     the plain per-sample recurrence, every operation in `dtype` (np.float64 or LD, the 64-bit-mantissa long double).
                   Shares no code with synth.preintegrate, the oracle or the kernel.
  tree_emulation   float64 in the order the comment above k_preint documents: batches of PRE_B = 24 samples, a pairwise tree
                   `slot a <- slot b o slot a` per batch, then the fold into the running (J, P); optionally the state chain by
                   the kernel's lane scans as well.  It exists to prove on the CPU that the bound below is attainable in float64
                   by that order, and to build records with seeded defects (`defect`).
  block_distance   5 x 5 table of per-3x3-block distances, the difference taken in LD.
  fixture          ONE batch of intervals shared by the CPU proof and the GPU test (lengths 0..50, the batch edges, fast
                   rotation, degenerate samples, first measurements drawn independently of the stream).
  floors           the float64 floor of the recurrence: float64 sequential against LD sequential, pooled over the fixture.
  violations       what of a record misses `distance <= MARGIN x floor`, exact equality where the floor is 0 -- the function the
                   GPU test asserts with and tests/test_preint_ref.py shows to reject seeded defects.
  sqrt_info_mp ..  the square-root information U = chol(cov^-1)^T of a record's covariance in 50 digits and the two measures
                   (per column, and E = max |U cov U^T - I|) the device's and the oracle's routines are held to.

Conventions: quaternions are (w, x, y, z) inside this module and [x y z w] in the returned dq, as in the record; the 15 states are
ordered P R V BA BG; record layout as vilsolve.h (VIL_IMU_CONST = 287)."""
import functools

import numpy as np

LD = np.longdouble
PRE_B = 24                      # samples per batch of k_preint
MARGIN = 16.0                   # a device operation order over a float64 floor (as tests/test_gpu_posegraph.py)
NOISE = (0.02065, 0.00519, 0.00667, 0.00088056)       # ACC_N GYR_N ACC_W GYR_W of the estimator's configuration (= preint.NOISE)
BLOCKS = ("P", "R", "V", "BA", "BG")
SEEDS = (0, 1, 2)
PLAIN_LENGTHS = tuple(range(0, 51)) + (71, 72, 73, 96, 97)
VARIANT_LENGTHS = (1, 7, 23, 24, 25, 49, 150)


# ---- the recurrence ---------------------------------------------------------------------------------------------------------
def _qmul(a, b):
    aw, ax, ay, az = a; bw, bx, by, bz = b
    return (aw * bw - ax * bx - ay * by - az * bz, aw * bx + ax * bw + ay * bz - az * by,
            aw * by + ay * bw + az * bx - ax * bz, aw * bz + az * bw + ax * by - ay * bx)


def _rotmat(q, T):
    """Rotation-matrix polynomial of a quaternion that need not have unit length (no division by its norm)."""
    w, x, y, z = q
    two = T(2)
    R = np.empty((3, 3), T)
    R[0, 0] = 1 - two * (y * y + z * z); R[0, 1] = two * (x * y - w * z); R[0, 2] = two * (x * z + w * y)
    R[1, 0] = two * (x * y + w * z); R[1, 1] = 1 - two * (x * x + z * z); R[1, 2] = two * (y * z - w * x)
    R[2, 0] = two * (x * z - w * y); R[2, 1] = two * (y * z + w * x); R[2, 2] = 1 - two * (x * x + y * y)
    return R


def _cross_matrix(v, T):
    S = np.zeros((3, 3), T)
    S[0, 1], S[0, 2], S[1, 0], S[1, 2], S[2, 0], S[2, 1] = -v[2], v[1], v[2], -v[0], -v[1], v[0]
    return S


def _normalised(q, T):
    n = np.sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3])
    return tuple(c / n for c in q)


def noise_diag(noise4, T):
    n = [T(x) * T(x) for x in noise4]
    return np.repeat(np.array([n[0], n[1], n[0], n[1], n[2], n[3]], T), 3)


def sample_maps(q, h, d0, d1, w, dt, nd, T, rr_normalised=False):
    """F (15 x 15), Q = V N V^T (15 x 15) of one sample and the two rotated accelerations.  q: delta_q at the start of the sample
    (unit), h = w dt / 2, d0 / d1 = a0 - ba / a1 - ba, w the mid-point rate.  The header's second quirk lives here: Rr and the
    rotated d1 use the UN-normalised product q (x) (1, h); `rr_normalised` is the seeded defect that normalises it first."""
    r = _qmul(q, (T(1), h[0], h[1], h[2]))
    if rr_normalised:
        r = _normalised(r, T)
    Rd, Rr = _rotmat(q, T), _rotmat(r, T)
    I3 = np.eye(3, dtype=T)
    A0, A1, Wx = _cross_matrix(d0, T), _cross_matrix(d1, T), _cross_matrix(w, T)
    G = I3 - Wx * dt                         # the rotation block of F
    RA0, RA1 = Rd @ A0, Rr @ A1
    RA1G = RA1 @ G
    dt2 = dt * dt
    q4, h2 = T(0.25), T(0.5)
    F = np.zeros((15, 15), T); V = np.zeros((15, 18), T)
    F[0:3, 0:3] = I3
    F[0:3, 3:6] = -q4 * RA0 * dt2 - q4 * RA1G * dt2
    F[0:3, 6:9] = I3 * dt
    F[0:3, 9:12] = -q4 * (Rd + Rr) * dt2
    F[0:3, 12:15] = q4 * RA1 * dt2 * dt
    F[3:6, 3:6] = G
    F[3:6, 12:15] = -I3 * dt
    F[6:9, 3:6] = -h2 * RA0 * dt - h2 * RA1G * dt
    F[6:9, 6:9] = I3
    F[6:9, 9:12] = -h2 * (Rd + Rr) * dt
    F[6:9, 12:15] = h2 * RA1 * dt * dt
    F[9:12, 9:12] = I3; F[12:15, 12:15] = I3
    V[0:3, 0:3] = q4 * Rd * dt2
    V[0:3, 3:6] = -q4 * RA1 * dt2 * h2 * dt
    V[0:3, 6:9] = q4 * Rr * dt2
    V[0:3, 9:12] = V[0:3, 3:6]
    V[3:6, 3:6] = h2 * I3 * dt; V[3:6, 9:12] = h2 * I3 * dt
    V[6:9, 0:3] = h2 * Rd * dt
    V[6:9, 3:6] = -h2 * RA1 * dt * h2 * dt
    V[6:9, 6:9] = h2 * Rr * dt
    V[6:9, 9:12] = V[6:9, 3:6]
    V[9:12, 12:15] = I3 * dt; V[12:15, 15:18] = I3 * dt
    return F, (V * nd) @ V.T, Rd @ d0, Rr @ d1, r


def _cast(T, *xs):
    return [np.asarray(x, np.float64).astype(T) for x in xs]


def preintegrate(dt, acc, gyr, acc0, gyr0, ba, bg, noise4, dtype):
    """(dp, dq [x y z w], dv, sum_dt, J 15 x 15, P 15 x 15) of one interval, the plain recurrence, everything in `dtype`."""
    T = dtype
    dt, acc, gyr, a0, g0, ba, bg = _cast(T, dt, acc, gyr, acc0, gyr0, ba, bg)
    nd = noise_diag(noise4, T)
    half = T(0.5)
    dp, dv, q, sum_dt = np.zeros(3, T), np.zeros(3, T), (T(1), T(0), T(0), T(0)), T(0)
    J, P = np.eye(15, dtype=T), np.zeros((15, 15), T)
    for s in range(len(dt)):
        h_t, a1, g1 = dt[s], acc[s], gyr[s]
        w = half * (g0 + g1) - bg
        h = w * h_t / 2
        F, Q, u0, u1, r = sample_maps(q, h, a0 - ba, a1 - ba, w, h_t, nd, T)
        ua = half * (u0 + u1)
        dp = dp + dv * h_t + half * ua * h_t * h_t
        dv = dv + ua * h_t
        q = _normalised(r, T)               # first quirk: delta_q is normalised after every sample
        J = F @ J
        P = F @ P @ F.T + Q
        sum_dt = sum_dt + h_t
        a0, g0 = a1, g1
    return dp, np.array([q[1], q[2], q[3], q[0]], T), dv, sum_dt, J, P


# ---- the kernel's order, float64 ---------------------------------------------------------------------------------------------
def tree_levels(nb):
    """[(st, pairs, wide)] of one batch of nb samples: the pair stride, the number of pairs and which of the kernel's two code
    paths the level takes (wide: 3 x 3 register blocks, when pairs x 50 tasks fill the 256 lanes)."""
    out, st = [], 1
    while st < nb:
        npair = (nb - st + 2 * st - 1) // (2 * st)
        out.append((st, npair, npair * 50 >= 256))
        st *= 2
    return out


def _scan(x, combine):
    """Inclusive Hillis-Steele scan over the lanes of one batch, offsets 1, 2, 4, 8, 16 as the kernel's shuffles; x: list per lane."""
    o = 1
    while o < PRE_B:
        x = [combine(x[l - o], x[l]) if l >= o else x[l] for l in range(len(x))]
        o *= 2
    return x


def tree_emulation(dt, acc, gyr, acc0, gyr0, ba, bg, noise4, scans=False, defect=None):
    """float64 in k_preint's documented order.  scans = False: the state chain runs sample by sample (the tree alone);
    True: as the kernel, a prefix product of the quaternion increments and two prefix sums per batch.
    defect: None, ("drop_qb", st, pair) -- the `+ Q_b` of that pair at that level of the first batch is left out --, or
    ("rr_normalised",) -- Rr and the rotated a1 - ba from the normalised product."""
    T = np.float64
    dt, acc, gyr, a0, g0, ba, bg = _cast(T, dt, acc, gyr, acc0, gyr0, ba, bg)
    nd = noise_diag(noise4, T)
    rrn = defect is not None and defect[0] == "rr_normalised"
    dp, dv, q, sum_dt = np.zeros(3), np.zeros(3), (1.0, 0.0, 0.0, 0.0), 0.0
    J, P = np.eye(15), np.zeros((15, 15))
    prev_a = np.vstack([a0[None], acc[:-1]]) if len(dt) else acc
    prev_g = np.vstack([g0[None], gyr[:-1]]) if len(dt) else gyr
    for b0 in range(0, len(dt), PRE_B):
        nb = min(PRE_B, len(dt) - b0)
        sl = slice(b0, b0 + nb)
        hb, w = dt[sl], 0.5 * (prev_g[sl] + gyr[sl]) - bg
        d0, d1 = prev_a[sl] - ba, acc[sl] - ba
        hh = w * hb[:, None] / 2
        Fs, Qs = [], []
        if scans:
            pre = _scan([(1.0, hh[l, 0], hh[l, 1], hh[l, 2]) for l in range(nb)], _qmul)
            qs = [_normalised(_qmul(q, (1.0, 0.0, 0.0, 0.0) if l == 0 else pre[l - 1]), T) for l in range(nb)]
            ua = np.zeros((nb, 3))
            for l in range(nb):
                F, Q, u0, u1, r = sample_maps(qs[l], hh[l], d0[l], d1[l], w[l], hb[l], nd, T, rrn)
                Fs.append(F); Qs.append(Q); ua[l] = 0.5 * (u0 + u1)
            iv = np.array(_scan(list(ua * hb[:, None]), np.add))
            isum = _scan(list(hb), lambda a, b: a + b)
            dvs = dv + (iv - ua * hb[:, None])                       # delta_v at the start of each sample
            ip = np.array(_scan(list(dvs * hb[:, None] + 0.5 * ua * hb[:, None] * hb[:, None]), np.add))
            dp, dv, q, sum_dt = dp + ip[-1], dv + iv[-1], _normalised(r, T), sum_dt + isum[-1]
        else:
            for l in range(nb):
                F, Q, u0, u1, r = sample_maps(q, hh[l], d0[l], d1[l], w[l], hb[l], nd, T, rrn)
                ua = 0.5 * (u0 + u1)
                dp = dp + dv * hb[l] + 0.5 * ua * hb[l] * hb[l]
                dv = dv + ua * hb[l]
                q = _normalised(r, T); sum_dt = sum_dt + hb[l]
                Fs.append(F); Qs.append(Q)
        for st, npair, _ in tree_levels(nb):
            for p in range(npair):
                sa, sb = 2 * st * p, 2 * st * p + st
                Tm = Fs[sb] @ Qs[sa]
                new_q = Tm @ Fs[sb].T
                if not (defect is not None and defect[0] == "drop_qb" and b0 == 0 and (st, p) == tuple(defect[1:])):
                    new_q = new_q + Qs[sb]
                Qs[sa] = new_q
                Fs[sa] = Fs[sb] @ Fs[sa]
        J = Fs[0] @ J
        P = (Fs[0] @ P) @ Fs[0].T + Qs[0]
    return dp, np.array([q[1], q[2], q[3], q[0]]), dv, sum_dt, J, P


# ---- records -----------------------------------------------------------------------------------------------------------------
def to_record(out, ba, bg):
    """(record 287, jacobian 15 x 15) in float64 from a preintegrate / tree_emulation result."""
    dp, dq, dv, sum_dt, J, P = [np.asarray(x, np.float64) for x in out]
    c = np.zeros(287)
    c[0:3], c[3:7], c[7:10], c[10:13], c[13:16], c[16] = dp, dq, dv, ba, bg, sum_dt
    for off, (r0, c0) in zip((17, 26, 35, 44, 53), ((0, 9), (0, 12), (3, 12), (6, 9), (6, 12))):
        c[off:off + 9] = J[r0:r0 + 3, c0:c0 + 3].ravel()
    c[62:] = P.ravel()
    return c, J.copy()


def block_distance(A, ref):
    """5 x 5 table, one entry per 3 x 3 block of a 15 x 15 matrix: max |A - ref| / max |ref| over the block, the difference taken in
    LD; where the reference block is all zero the entry is max |A| of the block."""
    d = np.abs(np.asarray(A).astype(LD) - np.asarray(ref).astype(LD)).reshape(5, 3, 5, 3).max(axis=(1, 3))
    m = np.abs(np.asarray(ref).astype(LD)).reshape(5, 3, 5, 3).max(axis=(1, 3))
    a = np.abs(np.asarray(A).astype(LD)).reshape(5, 3, 5, 3).max(axis=(1, 3))
    return np.where(m == 0, a, d / np.where(m == 0, 1, m)).astype(np.float64)


def _vec_rel(a, ref):
    """distance of a vector relative to the reference's largest component (absolute where the reference is all zero)"""
    d = float(np.abs(np.asarray(a).astype(LD) - ref).max()); m = float(np.abs(ref).max())
    return d / m if m > 0 else d


def distances(rec, jac, ref):
    """every output of one interval against its LD reference: {"J": 5 x 5, "P": 5 x 5, "dp", "dv" (relative to the vector's largest
    component), "dq" (absolute), "sum_dt" (relative)}"""
    dp, dq, dv, sum_dt, J, P = ref
    return {"J": block_distance(jac, J), "P": block_distance(rec[62:].reshape(15, 15), P), "dp": _vec_rel(rec[0:3], dp), "dv": _vec_rel(rec[7:10], dv),
            "dq": float(np.abs(rec[3:7].astype(LD) - dq).max()), "sum_dt": _vec_rel(rec[16:17], np.asarray([sum_dt], LD))}


# ---- the shared fixture ------------------------------------------------------------------------------------------------------
def _signals(rng, n, rate=200.0):
    """a smooth stream of the shape of preint.make_stream's: gravity plus slow sines plus sensor noise, dt jittered by 10 %"""
    tt = np.arange(n) / rate
    ph = rng.uniform(0, 2 * np.pi, (2, 3))
    acc = np.stack([0.8 * np.sin(1.3 * tt + ph[0, 0]), 0.6 * np.cos(0.9 * tt + ph[0, 1]), 9.8 + 0.4 * np.sin(2.1 * tt + ph[0, 2])], axis=1) + rng.normal(0, 0.05, (n, 3))
    gyr = np.stack([0.3 * np.sin(0.7 * tt + ph[1, 0]), 0.25 * np.cos(1.1 * tt + ph[1, 1]), 0.4 * np.sin(0.5 * tt + ph[1, 2])], axis=1) + rng.normal(0, 0.01, (n, 3))
    return np.full(n, 1.0 / rate) * rng.uniform(0.9, 1.1, n), acc, gyr


class Fixture:
    """start, dt, acc, gyr, acc0, gyr0, ba, bg as vpre_integrate takes them, plus per interval its length, variant and seed"""

    def __init__(self, start, dt, acc, gyr, acc0, gyr0, ba, bg, length, variant, seed):
        self.batch = (start, dt, acc, gyr, acc0, gyr0, ba, bg)
        self.length, self.variant, self.seed = length, variant, seed
        for a in self.batch:
            a.setflags(write=False)

    def __len__(self):
        return len(self.length)

    def interval(self, k):
        """the arguments of preintegrate / tree_emulation (without noise) for interval k"""
        start, dt, acc, gyr, acc0, gyr0, ba, bg = self.batch
        a, b = start[k], start[k + 1]
        return dt[a:b], acc[a:b], gyr[a:b], acc0[k], gyr0[k], ba[k], bg[k]

    def find(self, length, variant="plain", seed=0):
        return next(k for k in range(len(self)) if (self.length[k], self.variant[k], self.seed[k]) == (length, variant, seed))

    def subset(self, ks):
        """the batch holding only the intervals ks, in that order"""
        start, dt, acc, gyr, acc0, gyr0, ba, bg = self.batch
        idx = np.concatenate([np.arange(start[k], start[k + 1]) for k in ks] + [np.zeros(0, np.int64)]).astype(np.int64)
        st = np.concatenate([[0], np.cumsum([self.length[k] for k in ks])]).astype(np.int32)
        ks = list(ks)
        return st, dt[idx], acc[idx], gyr[idx], acc0[ks], gyr0[ks], ba[ks], bg[ks]


@functools.lru_cache(maxsize=None)
def fixture():
    """For each of three seeds: every length 0 .. 50 and 71, 72, 73, 96, 97 (plain); lengths 1, 7, 23, 24, 25, 49, 150 with the rates
    x 25 (fast) and with every fifth dt = 0 and the biases x 20 (degenerate).  acc0 / gyr0 are drawn independently of the stream,
    so a kernel that reads the previous interval's last sample instead of them computes something else."""
    dts, accs, gyrs, a0s, g0s, bas, bgs, length, variant, seed = [], [], [], [], [], [], [], [], [], []
    for sd in SEEDS:
        rng = np.random.default_rng(1000 + sd)
        for var, lengths in (("plain", PLAIN_LENGTHS), ("fast", VARIANT_LENGTHS), ("degenerate", VARIANT_LENGTHS)):
            for n in lengths:
                dt, acc, gyr = _signals(rng, n)
                ba, bg = rng.normal(0, 0.05, 3), rng.normal(0, 0.005, 3)
                a0, g0 = rng.normal(0, 3.0, 3) + np.array([0, 0, 9.8]), rng.normal(0, 0.5, 3)
                if var == "fast":
                    gyr, g0 = gyr * 25.0, g0 * 25.0
                if var == "degenerate":
                    dt[::5] = 0.0; ba, bg = ba * 20.0, bg * 20.0
                dts.append(dt); accs.append(acc); gyrs.append(gyr); a0s.append(a0); g0s.append(g0); bas.append(ba); bgs.append(bg)
                length.append(n); variant.append(var); seed.append(sd)
    start = np.concatenate([[0], np.cumsum(length)]).astype(np.int32)
    return Fixture(start, np.concatenate(dts), np.vstack(accs), np.vstack(gyrs), np.array(a0s), np.array(g0s), np.array(bas), np.array(bgs),
                   tuple(length), tuple(variant), tuple(seed))


@functools.lru_cache(maxsize=None)
def reference(dtype, noise4=NOISE, ks=None):
    """the recurrence in `dtype` on the intervals ks of the fixture (default: all), computed once per process"""
    fx = fixture()
    return tuple(preintegrate(*fx.interval(k), noise4, dtype) for k in (range(len(fx)) if ks is None else ks))


# ---- floor and check ---------------------------------------------------------------------------------------------------------
def pool(ds):
    """the largest distance per output over a list of `distances` results"""
    return {k: (np.max([d[k] for d in ds], axis=0) if k in ("J", "P") else max(d[k] for d in ds)) for k in ("J", "P", "dp", "dv", "dq", "sum_dt")}


@functools.lru_cache(maxsize=None)
def floors():
    """The float64 floor of every output: the float64 sequential recurrence's distance from the LD one, maximised over the fixture."""
    fx = fixture()
    ds = []
    for k, (r64, rld) in enumerate(zip(reference(np.float64), reference(LD))):
        rec, jac = to_record(r64, fx.batch[6][k], fx.batch[7][k])
        ds.append(distances(rec, jac, rld))
    return pool(ds)


def violations(rec, jac, ref, floor=None, margin=MARGIN):
    """What of one interval's record misses `distance <= margin x floor` -- or, where the floor is 0, equality with the float64
    rounding of the reference -- as a list of (output, distance, floor).  Empty: the record passes."""
    floor = floor or floors()
    d = distances(rec, jac, ref)
    dp, dq, dv, sum_dt, J, P = ref
    bad = []
    for name, A, R in (("J", jac, J), ("P", rec[62:].reshape(15, 15), P)):
        for i in range(5):
            for j in range(5):
                f = floor[name][i, j]
                blk = (slice(3 * i, 3 * i + 3), slice(3 * j, 3 * j + 3))
                ok = np.array_equal(np.asarray(A)[blk], R[blk].astype(np.float64)) if f == 0 else d[name][i, j] <= margin * f
                if not ok:
                    bad.append(("%s(%s,%s)" % (name, BLOCKS[i], BLOCKS[j]), d[name][i, j], f))
    for name, a, r in (("dp", rec[0:3], dp), ("dv", rec[7:10], dv), ("dq", rec[3:7], dq), ("sum_dt", rec[16:17], np.asarray([sum_dt], LD))):
        f = floor[name]
        ok = np.array_equal(a, np.asarray(r).astype(np.float64)) if f == 0 else d[name] <= margin * f
        if not ok:
            bad.append((name, d[name], f))
    return bad


def report(ds, meta, floor=None):
    """One line per output: floor, the worst distance, their ratio and the interval (length, variant, seed) where it occurs."""
    floor = floor or floors()
    lines, worst = [], 0.0
    def line(name, f, vals):
        nonlocal worst
        k = int(np.argmax(vals)); v = float(vals[k])
        if f > 0:
            worst = max(worst, v / f)
        lines.append("%-10s floor %.2e  distance %.2e  ratio %s  worst at length %d %s seed %d" % (name, f, v, "%.2f" % (v / f) if f > 0 else ("exact" if v == 0 else "NOT EXACT"), *meta[k]))
    for name in ("J", "P"):
        for i in range(5):
            for j in range(5):
                line("%s(%s,%s)" % (name, BLOCKS[i], BLOCKS[j]), floor[name][i, j], [d[name][i, j] for d in ds])
    for name in ("dp", "dq", "dv", "sum_dt"):
        line(name, floor[name], [d[name] for d in ds])
    return lines, worst


# ---- the square-root information of a record's covariance -------------------------------------------------------------------
WHITEN_LENGTHS = (3, 5, 24, 60, 400)          # plain intervals; 1 or 2 samples give covariances numpy's own route fails on


@functools.lru_cache(maxsize=None)
def whitening_batch():
    """one batch of plain intervals of WHITEN_LENGTHS samples, as vpre_integrate takes it"""
    rng = np.random.default_rng(77)
    parts = [_signals(rng, n) for n in WHITEN_LENGTHS]
    n = len(parts)
    start = np.concatenate([[0], np.cumsum(WHITEN_LENGTHS)]).astype(np.int32)
    return (start, np.concatenate([p[0] for p in parts]), np.vstack([p[1] for p in parts]), np.vstack([p[2] for p in parts]),
            rng.normal(0, 3.0, (n, 3)) + np.array([0, 0, 9.8]), rng.normal(0, 0.5, (n, 3)), rng.normal(0, 0.05, (n, 3)), rng.normal(0, 0.005, (n, 3)))


def lower_symmetric(cov):
    """The covariance every route is given: the record's lower triangle mirrored (the device and the oracle read only that triangle;
    the record's two triangles differ by roundings, and numpy's inverse and the 50-digit one would read both)."""
    L = np.tril(np.asarray(cov, np.float64).reshape(15, 15))
    return L + np.tril(L, -1).T


def sqrt_info_mp(cov):
    """U = chol(cov^-1)^T in 50-digit arithmetic (positive diagonal, so unique), as an mpmath matrix"""
    import mpmath as mp
    with mp.workdps(50):
        A = mp.matrix(cov.tolist())
        return mp.cholesky(A ** -1).T


def sqrt_info_numpy(cov):
    return np.linalg.cholesky(np.linalg.inv(cov)).T


def column_distance(U, U_ref, cols):
    """per column c of cols: max |U[:, c] - U_ref[:, c]| / max |U_ref[:, c]|, the difference taken in 50 digits"""
    import mpmath as mp
    out = []
    with mp.workdps(50):
        for c in cols:
            d = max(abs(mp.mpf(float(U[r, c])) - U_ref[r, c]) for r in range(15))
            out.append(float(d / max(abs(U_ref[r, c]) for r in range(15))))
    return np.array(out)


def whitening_error(U, cov):
    """E = max |U cov U^T - I| in 50 digits"""
    import mpmath as mp
    with mp.workdps(50):
        Um, Cm = mp.matrix(np.asarray(U, np.float64).tolist()), mp.matrix(cov.tolist())
        R = Um * Cm * Um.T - mp.eye(15)
        return float(max(abs(R[i, j]) for i in range(15) for j in range(15)))
