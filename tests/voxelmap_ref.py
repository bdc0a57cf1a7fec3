"""Test infrastructure: a sequential NumPy restatement of the target voxel map of include/vilvgicp.h (GaussianVoxelMap::create_voxelmap with
ADDITIVE voxels, gicp/fast_vgicp_voxel.hpp:107-159) and the fixtures of tests/test_voxelmap_ref.py and tests/test_gpu_voxelmap.py.

The contract: key per point = pack_key(floor(p / res - 0.5)) per axis with p the float coordinate as a double; voxels numbered in the order
of their first point; num, mean (3) and cov (9) are sequential double sums in ascending point index starting from 0.0; then mean and cov
are divided by num, and wsq = sqrt(num).  pack_key / hash_key are written here from their definition and share no code with the library."""
import numpy as np

F = np.float32
RES = 0.5
M21 = 0x1FFFFF
GOLD = 0x9E3779B97F4A7C15


def pack_key(x, y, z):
    """21 bits per axis, two's complement, x in the high bits: a non-negative 63-bit integer."""
    return ((int(x) & M21) << 42) | ((int(y) & M21) << 21) | (int(z) & M21)


def hash_key(k):
    """High 32 bits of the 64-bit product with the golden-ratio constant."""
    return ((int(k) * GOLD) & 0xFFFFFFFFFFFFFFFF) >> 32


def voxel_coords(xyz, res=RES):
    p = np.asarray(xyz, F).astype(np.float64)
    return np.floor(p / np.float64(res) - 0.5).astype(np.int64)


def point_keys(xyz, res=RES):
    return np.array([pack_key(*c) for c in voxel_coords(xyz, res)], np.int64).reshape(-1)


def build(xyz, cov9, res=RES, order=None):
    """The host loop, statement by statement.  order: the sequence in which the points are ADDED (default: ascending index) -- only the
    order fixture's self-check passes another one; the numbering is by first point of that sequence.
    Returns dict(keys int64, num int32, mean (nv, 3), cov (nv, 9), wsq (nv))."""
    xyz = np.ascontiguousarray(xyz, F).reshape(-1, 3)
    cov9 = np.ascontiguousarray(cov9, np.float64).reshape(-1, 9)
    assert len(xyz) == len(cov9) and np.isfinite(xyz).all()
    p = xyz.astype(np.float64)
    pk = point_keys(xyz, res)
    index, keys, num, mean, cov = {}, [], [], [], []
    for i in (range(len(xyz)) if order is None else order):
        k = int(pk[i])
        v = index.get(k)
        if v is None:
            v = index[k] = len(keys)
            keys.append(k); num.append(0); mean.append(np.zeros(3)); cov.append(np.zeros(9))
        num[v] += 1
        mean[v] += p[i]                      # elementwise double adds, the first one 0.0 + p
        cov[v] += cov9[i]
    nv = len(keys)
    num = np.array(num, np.int32).reshape(nv)
    mean = np.array(mean, np.float64).reshape(nv, 3) / num[:, None].astype(np.float64)
    cov = np.array(cov, np.float64).reshape(nv, 9) / num[:, None].astype(np.float64)
    return dict(keys=np.array(keys, np.int64).reshape(nv), num=num, mean=mean, cov=cov, wsq=np.sqrt(num.astype(np.float64)))


def raw(a):
    return np.ascontiguousarray(a).view(np.uint8)


def same_map(a, b):
    """Every field equal in dtype, shape and raw bytes (so -0.0 differs from +0.0)."""
    return all(a[f].dtype == b[f].dtype and a[f].shape == b[f].shape and np.array_equal(raw(a[f]), raw(b[f])) for f in ("keys", "num", "mean", "cov", "wsq"))


# ---- fixtures ---------------------------------------------------------------------------------------------------------------------
def random_cov(rng, n):
    """Full-mantissa doubles of either sign with magnitudes from 1e-3 to 1e3: sums of them round at every addition."""
    return (rng.uniform(1.0, 2.0, (n, 9)) * 10.0 ** rng.uniform(-3, 3, (n, 9)) * rng.choice([-1.0, 1.0], (n, 9))).astype(np.float64)


def plain_cov(n):
    """The same well-conditioned covariance for every point (the alignment fixtures)."""
    return np.tile(np.array([0.02, 0.001, 0.0, 0.001, 0.03, 0.002, 0.0, 0.002, 0.025]), (n, 1))


def boundary_cloud(res=RES):
    """Per axis and for k = -3 ... 3: a coordinate of exactly k * res + res / 2 (where p / res - 0.5 is the integer k) and its two float
    neighbours; the other two coordinates sit inside a voxel."""
    pts = []
    for axis in range(3):
        for k in range(-3, 4):
            c = F(k * res + 0.5 * res)
            for v in (np.nextafter(c, F(-np.inf)), c, np.nextafter(c, F(np.inf))):
                p = [F(0.1), F(0.1), F(0.1)]; p[axis] = v
                pts.append(p)
    return np.array(pts, F)


def zero_cloud():
    """+-0.0 in every combination of the three coordinates, -0.0 first: all in one voxel; a sum that starts from its first term instead of
    0.0 keeps the sign of -0.0."""
    z = [F(-0.0), F(0.0)]
    return np.array([[a, b, c] for a in z for b in z for c in z], F)


def in_voxel(rng, coords, res=RES):
    """One point strictly inside each of the given voxels (coordinates (k + 1 +- 0.4) * res)."""
    coords = np.asarray(coords, np.float64).reshape(-1, 3)
    return ((coords + 1.0 + rng.uniform(-0.4, 0.4, coords.shape)) * res).astype(F)


def order_fixture(n_total=600, seed=5):
    """Voxel A interleaved with two others, A B A C A B A C ...: n_total = 600 gives A 300 points, its run crossing the 256-thread block
    edge in the point order.  Covariances are random_cov, so the order of the additions shows in the bits (order_matters checks it)."""
    rng = np.random.default_rng(seed)
    which = np.array([0 if i % 2 == 0 else (1 if i % 4 == 1 else 2) for i in range(n_total)])
    coords = np.array([[2, -1, 0], [-3, 4, 1], [7, 7, -2]])[which]
    return in_voxel(rng, coords), random_cov(rng, n_total), which


def order_matters(xyz, cov9, which, voxel=0):
    """True when adding `voxel`'s points in REVERSED order changes at least one bit of its covariance sum."""
    n = len(xyz)
    idx = [i for i in range(n) if which[i] == voxel]
    rev = iter(reversed(idx))
    order = [next(rev) if which[i] == voxel else i for i in range(n)]
    a, b = build(xyz, cov9), build(xyz, cov9, order=order)
    va, vb = list(a["keys"]).index(point_keys(xyz[idx[:1]])[0]), list(b["keys"]).index(point_keys(xyz[idx[:1]])[0])
    assert a["num"][va] == b["num"][vb] == len(idx)
    return not np.array_equal(raw(a["cov"][va]), raw(b["cov"][vb]))


def collision_coords(count=48, radius=40, bits=12):
    """`count` voxel coordinates of the cube [-radius, radius]^3, in scan order, whose keys share the low `bits` bits of hash_key: they
    collide in any table of up to 2^bits slots.  Brute force over the cube; the bucket is the fullest one."""
    r = np.arange(-radius, radius + 1, dtype=np.int64)
    x, y, z = [g.ravel() for g in np.meshgrid(r, r, r, indexing="ij")]
    k = ((x & M21) << 42) | ((y & M21) << 21) | (z & M21)
    h = ((k.astype(np.uint64) * np.uint64(GOLD)) >> np.uint64(32)).astype(np.int64) & ((1 << bits) - 1)
    bucket = int(np.bincount(h, minlength=1 << bits).argmax())
    pick = np.nonzero(h == bucket)[0][:count]
    assert len(pick) == count, "the cube holds only %d colliding keys" % len(pick)
    return np.stack([x[pick], y[pick], z[pick]], axis=1)


def collision_fixture(per_key=1, seed=6):
    """48 colliding voxels with per_key points each (key-major: the second points follow all the first ones)."""
    rng = np.random.default_rng(seed)
    coords = np.tile(collision_coords(), (per_key, 1))
    return in_voxel(rng, coords), random_cov(rng, len(coords)), coords


def population_fixture(kind, seed=7):
    rng = np.random.default_rng(seed)
    if kind == "one_voxel":
        coords = np.tile([[1, 2, 3]], (2049, 1))
    elif kind == "all_own":
        j = np.arange(3000)
        coords = np.stack([j % 20 - 10, (j // 20) % 20 - 10, j // 400], axis=1)
    elif kind == "counts_1_to_60":                       # voxel j holds j points, shuffled: wsq for every count
        coords = np.concatenate([np.tile([[j, -j, 5]], (j, 1)) for j in range(1, 61)])
        coords = coords[rng.permutation(len(coords))]
    else:
        raise ValueError(kind)
    return in_voxel(rng, coords), random_cov(rng, len(coords))
