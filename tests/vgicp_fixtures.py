"""Fixtures of tests/test_vgicp_ref.py and tests/test_gpu_vgicp_ref.py, all built from seeds.  Each names the smallest shape at which its
kernel path of csrc/vilvgicp.hip can go wrong; docs/vgicp.md has the list."""
import functools
import itertools

import numpy as np

import vgicp_ref as ref
import voxelmap_ref as vr

F = np.float32
MODES = (ref.DIRECT1, ref.DIRECT7, ref.DIRECT27)


def rotation(axis, angle):
    a = np.asarray(axis, np.float64); a = a / np.linalg.norm(a)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * K @ K


def isometry(R, t):
    T = np.eye(4); T[:3, :3] = R; T[:3, 3] = t
    return T


def cov_with_condition(rng, n, cond):
    """n symmetric positive definite 3 x 3 (n x 9) with eigenvalues (1, 1, 1 / cond) in a random frame."""
    out = np.zeros((n, 9))
    for i in range(n):
        Q = rotation(rng.normal(size=3), rng.uniform(0, np.pi))
        out[i] = (Q @ np.diag([1.0, 1.0, 1.0 / cond]) @ Q.T).reshape(9)
    return out


# ---- edges: the transformed coordinate on and next to a cell edge (vox_coord's reciprocal and its fallback) -----------------------------
EDGE_RES = (0.5, 0.3, 0.1, 0.7, 1.0)
EDGE_K = (-100000, -37, -3, -1, 0, 1, 2, 41, 99999)
EDGE_J = range(-64, 65)
EDGE_RES_WITH_H = 0.1            # the edge cases are judged on the error alone (it tells which voxel was hit); this resolution also with H / b


def edge_centre(k, res):
    """c = fl(k * res + res / 2): where x / res - 0.5 is about the integer k; and the spacing of the doubles there."""
    c = float(k) * res + res / 2
    return c, float(np.spacing(np.float64(abs(c))))


@functools.lru_cache(maxsize=None)
def edges(axis, res, k):
    """Source points (j u, y, z), j = -64 ... 64, as float32; T = a translation by c along `axis`; the transformed coordinate c + j u is exact
    in double with or without fused multiply-adds (exact_edge_sums counts).  Target: one point in voxel k and one in voxel k - 1 of that axis,
    with different covariances, so the error tells which was hit.  The other two coordinates sit mid-voxel 0."""
    c, u = edge_centre(k, res)
    sx = np.zeros((len(EDGE_J), 3), F) + F(res)                       # q = 0.5: the middle of voxel 0
    sx[:, axis] = np.array([j * u for j in EDGE_J], np.float64).astype(F)
    t = np.zeros(3); t[axis] = c
    tx = np.zeros((2, 3), F) + F(res)
    tx[0, axis] = F((k + 1) * res); tx[1, axis] = F(k * res)         # q = k + 0.5 and k - 0.5
    tc = np.array([[0.02, 0.001, 0.0, 0.001, 0.03, 0.002, 0.0, 0.002, 0.025], [0.3, 0.0, 0.01, 0.0, 0.2, 0.0, 0.01, 0.0, 0.5]])
    sc = vr.plain_cov(len(sx))
    P = ref.Problem(tx, tc, sx, sc, res)
    assert [tuple(c) for c in vr.voxel_coords(tx, res)[:, axis:axis + 1]] == [(k,), (k - 1,)]
    return P, isometry(np.eye(3), t)


def exact_edge_sums(axis, res, k):
    """(samples, inexact): j u as float32 and c + j u as double against the exact rationals."""
    from fractions import Fraction
    P, T = edges(axis, res, k)
    c, u = edge_centre(k, res)
    bad = 0
    for j, a in zip(EDGE_J, P.sx[:, axis].astype(np.float64).tolist()):
        bad += (Fraction(a) != j * Fraction(u)) or (Fraction(c + a) != Fraction(c) + Fraction(a))
    return len(P.sx), int(bad)


def reciprocal_coord(x, res):
    """The mutant of item 1: x * fl(1 / res) instead of x / res, without the fallback."""
    return int(np.floor(x * (1.0 / res) - 0.5))


# ---- offsets: one cluster per neighbour offset ---------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def offsets_fixture(seed=11):
    """27 clusters 7 voxels apart, centres in {-7, 0, 7}^3 in a shuffled order (negative coordinates, the origin straddled).  In cluster o
    the one source point sits in the centre voxel and the only occupied voxel near it is centre + o; every cluster has its own covariance."""
    rng = np.random.default_rng(seed)
    offs = sorted(ref.offsets(ref.DIRECT27))
    centres = np.array(list(itertools.product((-7, 0, 7), repeat=3)))[rng.permutation(27)]
    tx = vr.in_voxel(rng, centres + np.array(offs), 0.5)
    sx = vr.in_voxel(rng, centres, 0.5)
    tc = cov_with_condition(rng, 27, 1e3) * rng.uniform(0.01, 0.1, (27, 1)); sc = cov_with_condition(rng, 27, 1e3) * rng.uniform(0.01, 0.1, (27, 1))
    T = isometry(rotation([0.3, -0.2, 0.9], 2e-3), [0.004, -0.003, 0.002])
    sx = ((sx.astype(np.float64) - T[:3, 3]) @ T[:3, :3]).astype(F)     # T sx = the drawn point, up to float32
    return ref.Problem(tx, tc, sx, sc, 0.5), T, offs


DIRECT7_MOVED = frozenset(ref.offsets(ref.DIRECT7) - {(0, 1, 0)} | {(1, 1, 0)})
# one DIRECT27 axis decoded in the wrong order.  Exchanging two axes gives the same SET of offsets and changes nothing observable; the
# wrong order that shows is that of the two operations of the middle axis: (o % 3) / 3 in place of (o / 3) % 3
DIRECT27_WRONG_ORDER = tuple((o // 9 - 1, (o % 3) // 3 - 1, o % 3 - 1) for o in range(27))


# ---- blocks: the per-slot formula and the two reductions ------------------------------------------------------------------------------
BLOCK_CASES = (  # (name, mode, source points, rotation angle, translation scale, condition of the covariances)
    ("one", 1, 1, 1.0, 20.0, 1e3), ("n255", 1, 255, 0.01, 5.0, 1.0), ("n256", 1, 256, 1.0, 20.0, 1e3), ("n257", 1, 257, 3.0, 10.0, 1e6),
    ("n513", 1, 513, 3.0, 20.0, 1e3), ("d7", 7, 40, 1.0, 20.0, 1e6), ("d27", 27, 40, 3.0, 5.0, 1e3))


@functools.lru_cache(maxsize=None)
def blocks_target(seed=21):
    """6 x 6 x 4 occupied voxels around the origin, voxel j with 1 + j mod 60 points: every sqrt(num) from 1 to 60 appears."""
    rng = np.random.default_rng(seed)
    cells = np.array(list(itertools.product(range(-3, 3), range(-3, 3), range(-2, 2))))
    coords = np.concatenate([np.tile(c, (1 + j % 60, 1)) for j, c in enumerate(cells)])
    coords = coords[rng.permutation(len(coords))]
    tx = vr.in_voxel(rng, coords, 0.5)
    third = len(tx) // 3
    tc = np.concatenate([cov_with_condition(rng, third, 1.0), cov_with_condition(rng, third, 1e3), cov_with_condition(rng, len(tx) - 2 * third, 1e6)]) * 0.05
    return tx, tc[rng.permutation(len(tx))]


@functools.lru_cache(maxsize=None)
def blocks(name):
    _, mode, n, angle, tscale, cond = next(c for c in BLOCK_CASES if c[0] == name)
    rng = np.random.default_rng(sum(map(ord, name)))
    tx, tc = blocks_target()
    T = isometry(rotation(rng.normal(size=3), angle), rng.uniform(-1, 1, 3) * tscale)
    world = rng.uniform([-1.45, -1.45, -0.95], [1.45, 1.45, 0.95], (n, 3))                 # inside the block of occupied voxels
    sx = ((world - T[:3, 3]) @ T[:3, :3]).astype(F)
    sc = cov_with_condition(rng, n, cond) * 0.05
    return ref.Problem(tx, tc, sx, sc, 0.5), T, mode


# ---- two_slots: the grid-stride loop of k_vgicp_align ----------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def two_slots(seed=31):
    """2 430 source points in DIRECT27: 65 610 slots, the first size above 128 x 512 at which a thread of k_vgicp_align takes two slots."""
    rng = np.random.default_rng(seed)
    tx, tc = blocks_target()
    T = isometry(rotation([0.1, 0.7, -0.4], 0.01), [0.02, -0.015, 0.01])
    world = rng.uniform([-1.4, -1.4, -0.9], [1.4, 1.4, 0.9], (2430, 3))
    sx = ((world - T[:3, 3]) @ T[:3, :3]).astype(F)
    return tx, tc, sx, vr.plain_cov(2430), T


# ---- far: a voxel coordinate beyond the 21 bits of pack_key -----------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def far():
    """Transformed voxel coordinates 2^21 + 3 and 3 - 2^21 on the x axis; the target has a voxel at coordinate 3: an Eigen::Vector3i key
    finds nothing, a key that keeps 21 bits per axis finds voxel 3."""
    res = 0.5
    tx = np.array([[(3 + 1) * res, res, res]], F)
    sx = np.array([[((1 << 21) + 3 + 1) * res, res, res], [(3 - (1 << 21) + 1) * res, res, res]], F)
    P = ref.Problem(tx, vr.plain_cov(1), sx, vr.plain_cov(2), res)
    assert [ref.voxel_coord(float(x), res)[0] for x in sx[:, 0]] == [(1 << 21) + 3, 3 - (1 << 21)] and vr.voxel_coords(tx, res)[0, 0] == 3
    return P, np.eye(4)


# ---- covariance fixtures ---------------------------------------------------------------------------------------------------------------
K = 20


@functools.lru_cache(maxsize=None)
def lattice():
    """8 x 8 dyadic lattices (spacing 1/4) on the three axis planes, 64 apart: every sum is exact, the normal is the axis."""
    g = np.array(list(itertools.product(range(8), repeat=2)), np.float64) / 4
    pts, axes = [], []
    for axis in range(3):
        p = np.zeros((64, 3)); p[:, [a for a in range(3) if a != axis]] = g; p[:, (axis + 1) % 3] += 64.0 * (axis + 1)
        pts.append(p); axes += [axis] * 64
    return np.concatenate(pts).astype(F), np.array(axes)


@functools.lru_cache(maxsize=None)
def tie(swapped=False):
    """Query 0 at the origin with 18 in-plane neighbours nearer than 2 (itself included: 19), then two candidates at squared distance exactly 4:
    index 1 in the plane, index 2 out of it (swapped: the other way round).  The 20th neighbour is the one with the smaller index."""
    near = [(i / 2, j / 2, 0.0) for i, j in itertools.product(range(2, -2, -1), range(-2, 3)) if (i, j) != (0, 0)][:18]       # x from 1 down: lopsided
    assert len(near) == 18
    a, b = (2.0, 0.0, 0.0), (0.0, 0.0, 2.0)
    pts = [(0.0, 0.0, 0.0)] + ([b, a] if swapped else [a, b]) + near
    return np.array(pts, F)


def _normal(C):
    w, V = np.linalg.eigh(np.array([[float(v) for v in r] for r in C]))
    return V[:, 0] * np.sign(V[np.argmax(np.abs(V[:, 0])), 0])


@functools.lru_cache(maxsize=None)
def unfused(seed=0):
    """Query 0, 18 near in-plane points, then B (index 19, out of plane) and A (index 20, in the plane) at almost the same distance: the unfused
    float32 sum puts A first, each contracted form puts B first or ties them (B has the smaller index).  Found by a seeded search: B's z is
    stepped through neighbouring floats."""
    for s in range(seed, seed + 400):
        rng = np.random.default_rng(s)
        q = rng.uniform(-1, 1, 3).astype(F)
        near = (q + np.column_stack([rng.uniform(0.0, 0.5, 18), rng.uniform(-0.3, 0.3, 18), rng.normal(0, 1e-3, 18)])).astype(F)
        A = (q + np.array([rng.uniform(0.6, 0.8), rng.uniform(0.6, 0.8), 0.0])).astype(F)
        dA = float(ref.sqdist32(q, A[None])[0])
        zb = np.sqrt(max(dA - 0.3 ** 2 - 0.2 ** 2, 0.0))
        B0 = (q + np.array([-0.3, 0.2, zb])).astype(F)
        cand = np.tile(B0, (801, 1))
        z = B0[2]
        zs = [z]
        for _ in range(400):
            zs.append(np.nextafter(zs[-1], F(np.inf)))
        lo = [z]
        for _ in range(400):
            lo.append(np.nextafter(lo[-1], F(-np.inf)))
        cand[:, 2] = np.array(lo[:0:-1] + zs, F)
        plain = ref.sqdist32(q, cand)
        ok = plain > ref.sqdist32(q, A[None])[0]
        for form in ("second", "third", "both"):
            ok &= ref.sqdist32(q, cand, form) <= ref.sqdist32(q, A[None], form)[0]
        if ok.any():
            B = cand[np.nonzero(ok)[0][0]]
            return np.vstack([q[None], near, B[None], A[None]]).astype(F)
    raise AssertionError("no unfused pair found")


TILTED = ((1e-6, 20, 0.0), (1e-2, 21, 0.0), (0.5, 257, 0.0), (0.9, 300, 0.0), (1e-2, 21, 1000.0))      # (l1 / l2, points, shift); 257 crosses the 256-candidate tile


@functools.lru_cache(maxsize=None)
def tilted(ratio, n, shift=0.0):
    """A noisy plane at a random tilt: in-plane extents 2 x 1, thickness sqrt(ratio) of the narrower one; optionally 1 000 m away."""
    rng = np.random.default_rng(int(1000 * ratio) + n)
    local = np.column_stack([rng.uniform(-1, 1, n) * 2.0, rng.uniform(-1, 1, n), rng.uniform(-1, 1, n) * np.sqrt(ratio)])
    R = rotation(rng.normal(size=3), rng.uniform(0.2, 2.5))
    return (local @ R.T + shift).astype(F)


def degenerate(kind):
    if kind == "collinear":
        return (np.arange(24)[:, None] * np.array([[0.25, 0.5, -0.125]])).astype(F)
    if kind == "coincident":
        return np.tile(np.array([[1.5, -2.25, 0.75]], F), (20, 1))
    raise ValueError(kind)


# ---- alignment: a corner of three wall patches ---------------------------------------------------------------------------------------------
def _walls(rng, n_per_wall, origin, noise=0.01):
    pts, cov = [], []
    for axis in range(3):
        p = rng.uniform(0.0, 4.0, (n_per_wall, 3)); p[:, axis] = rng.normal(0, noise, n_per_wall)
        c = np.eye(3); c[axis, axis] = 1e-3
        pts.append(p + np.array(origin)); cov += [c] * n_per_wall
    return np.concatenate(pts), np.array(cov)


NEAR, AWAY = (0.13, 0.21, 0.17), (30.13, -19.79, 10.17)
T_TRUE = isometry(rotation([0.2, -0.5, 0.8], 0.03), [0.08, -0.05, 0.06])


@functools.lru_cache(maxsize=None)
def corner(origin=NEAR, seed=41, n_source=150):
    """Target: about 800 points on three orthogonal 4 m wall patches with their corner at `origin`; source: 150 other points of the same
    walls, moved by T_TRUE^-1.  Far from the origin of the frame a rotation step is strongly non-linear: that is where trials get rejected."""
    rng = np.random.default_rng(seed)
    tx, tc = _walls(rng, 267, origin)
    sw, sc = _walls(rng, n_source // 3, origin)
    R, t = T_TRUE[:3, :3], T_TRUE[:3, 3]
    sx = (sw - t) @ R                                               # R^T (p - t)
    sc = np.array([R.T @ c @ R for c in sc])
    return ref.Problem(tx.astype(F), tc.reshape(-1, 9), sx.astype(F), sc.reshape(-1, 9), 0.5)


DEFAULTS = dict(neighbor_mode=1, optimizer=ref.LM, max_iterations=64, lm_max_iterations=10, rotation_epsilon=2e-3, transformation_epsilon=5e-4, lm_init_lambda_factor=1e-9)
# found by a seeded search over guesses (float64 route): 6 rejected trials on the way; two rejections in a row at the third iteration
POOR_GUESS = isometry(rotation([1.1, 1.3, 0.7], 0.02), [0.84, -0.75, -0.17])
BUDGET_GUESS = isometry(rotation([-0.5, 0.1, -0.3], 0.009), [-0.03, 0.05, 0.0])
ALIGN_CASES = {
    "nominal_lm": (NEAR, np.eye(4), {}),
    "nominal_gn": (NEAR, np.eye(4), dict(optimizer=ref.GN)),
    "poor_guess": (AWAY, POOR_GUESS, {}),
    "small_budget": (AWAY, BUDGET_GUESS, dict(lm_max_iterations=2, lm_init_lambda_factor=1e-12)),
    "one_iteration": (NEAR, np.eye(4), dict(max_iterations=1)),
    "two_iterations": (NEAR, np.eye(4), dict(max_iterations=2)),
    "direct7": (NEAR, np.eye(4), dict(neighbor_mode=7)),
}


def align_case(name):
    origin, guess, kw = ALIGN_CASES[name]
    return corner(origin), guess, dict(DEFAULTS, **kw)


@functools.lru_cache(maxsize=None)
def aligned(name, arith="mp"):
    """The restatement's alignment of a case, once per process."""
    P, guess, opts = align_case(name)
    return ref.align(P, guess, opts, ref.MP if arith == "mp" else ref.F64)


# ---- the judge applied: one set of functions for the oracle, the device and the mutants -----------------------------------------------------
ULP = 2.0 ** -52
T2_SHIFT = np.array([0.01, -0.005, 0.002])
COV_CLOUDS = dict(lattice=lambda: lattice()[0], tie=lambda: tie(False), tie_swapped=lambda: tie(True), unfused=unfused,
                  **{"tilted%d" % i: (lambda c=c: tilted(*c)) for i, c in enumerate(TILTED)})


def second_transform(T):
    T2 = np.array(T, np.float64); T2[:3, 3] += T2_SHIFT
    return T2


def expected_lin(P, T, mode, want_H=True):
    """(the 50-digit linearisation, the float64 floor per quantity), once per process."""
    key = ("expected", np.ascontiguousarray(T, np.float64).tobytes(), mode, want_H)
    if key not in P._corr:
        m = ref.linearize(P, T, mode, ref.MP, want_H)
        P._corr[key] = (m, ref.lin_floor(P, T, mode, m, want_H) if m["n"] else {})
    return P._corr[key]


def expected_err2(P, T, mode):
    """(the 50-digit error at second_transform(T) on the correspondences of the linearisation at T, its float64 floor)."""
    key = ("expected2", np.ascontiguousarray(T, np.float64).tobytes(), mode)
    if key not in P._corr:
        T2 = second_transform(T)
        e = ref.compute_error(P, T2, expected_lin(P, T, mode)[0], ref.MP)
        fl = max(abs(float(ref.compute_error(P, T2, ref.linearize(P, T, mode, A, False), A, order=order) - e)) for A, order in ref.F64_ROUTES)
        P._corr[key] = (e, fl)
    return P._corr[key]


def judge_values(got, P, T, mode, want_H=True):
    """got = (err, H or None, b or None, n) of any implementation -> (passes, {quantity: (distance, floor, ok)})."""
    m, fl = expected_lin(P, T, mode, want_H)
    assert not any(m["open"]), "the fixture has an open slot"
    e, H, b, n = got
    if n != m["n"]:
        return False, {"n": (n, m["n"], False)}
    if n == 0:
        return (e == 0.0 and (H is None or not np.asarray(H).any())), {}
    assert all(v > 0 for v in fl.values()), fl
    d = ref.distance((e, None if not want_H else np.asarray(H).tolist(), None if not want_H else np.asarray(b).tolist()), (m["err"], m["H"] if want_H else None, m["b"]))
    v = ref.verdict(d, fl)
    return all(x[2] for x in v.values()), v


def load(reg, P):
    reg.set_target(P.tx, P.tc, P.res); reg.set_source(P.sx, P.sc)


def judge_linearize(reg, P, T, mode, want_H=True, second=False, tag=""):
    """An implementation behind the Vgicp wrapper (already loaded with P) through the judge; second: also compute_error at the second transform."""
    e, H, b, n = reg.linearize(T, mode, jac=want_H)
    ok, v = judge_values((e, H, b, n), P, T, mode, want_H)
    report(tag, v)
    assert ok, (tag, v)
    if second and n:
        e2, fl2 = expected_err2(P, T, mode)
        got = reg.compute_error(second_transform(T))
        d = abs(float(ref.mp.mpf(got) - e2))
        report(tag + " err2", {"err": (d, fl2, d <= ref.MARGIN * fl2)})
        assert fl2 > 0 and d <= ref.MARGIN * fl2, (tag, d, fl2)
    return v


def report(tag, v):
    """Prints the figures of one case (pytest -s shows them)."""
    print("vgicp-ref", tag, {q: "%.2e/%.2e" % (x[0], x[1]) for q, x in v.items()})


def check_degenerate(C):
    """The invariants of a PLANE-regularised covariance, for clouds whose normal is not defined."""
    C = np.asarray(C, np.float64).reshape(-1, 3, 3)
    assert np.isfinite(C).all()
    assert np.abs(C - C.transpose(0, 2, 1)).max() <= ULP
    assert np.abs(np.trace(C, axis1=1, axis2=2) - 2.001).max() <= 4 * 2 * ULP          # 4 ulp of 2.001
    assert np.abs(np.linalg.eigvalsh(C) - np.array([1e-3, 1.0, 1.0])).max() <= 1e-12


@functools.lru_cache(maxsize=None)
def expected_cov(name):
    """(the 50-digit covariances, the relative gaps, the float64 floor clamped below at 8 ulp of 1)."""
    xyz = COV_CLOUDS[name]()
    Cm, gaps = ref.covariances(xyz, K, ref.MP)
    C64, _ = ref.covariances(xyz, K, ref.F64)
    return Cm, gaps, max(max(ref.cov_distance(C64, Cm)), 8 * ULP)


def judge_cov(got, name):
    """got: (n, 9) or nested 3 x 3 -> (passes, the largest distance, the floor)."""
    Cm, _, fl = expected_cov(name)
    got = np.asarray([[[float(v) for v in r] for r in C] for C in got] if not isinstance(got, np.ndarray) else got, np.float64).reshape(-1, 3, 3)
    d = max(ref.cov_distance(got.tolist(), Cm))
    return d <= ref.MARGIN * fl, d, fl


def summary_of(a):
    """A restatement alignment as what vgicp_align returns."""
    return dict(T=ref.to_np(a["T"]), iterations=a["iterations"], converged=a["converged"], lm_failed=a["lm_failed"], n_correspondences=a["n_correspondences"],
                final_error=float(a["final_error"]), final_hessian=ref.to_np(a["final_hessian"]))


def summary_from(T, s):
    return dict(T=np.array(T), iterations=s.iterations, converged=s.converged, lm_failed=s.lm_failed, n_correspondences=s.n_correspondences,
                final_error=s.final_error, final_hessian=np.array(s.final_hessian).reshape(6, 6))


@functools.lru_cache(maxsize=None)
def align_floors(name):
    """Float64 loop against the 50-digit loop: T (clamped below at iterations x 2^-52 x (1 + max |t|): the rounding of the state at each
    composition), final_error, final_hessian."""
    m, f = aligned(name, "mp"), aligned(name, "f64")
    assert m["decisions"] == f["decisions"]
    with ref.mp.workdps(ref.DPS):
        dist = lambda got, want: float(max(abs(ref.mp.mpf(float(g)) - w) for gr, wr in zip(got, want) for g, w in zip(gr, wr)))
        fs = summary_of(f)
        tmax = max(abs(float(m["T"][r][3])) for r in range(3))
        return dict(T=max(dist(fs["T"].tolist(), m["T"]), m["iterations"] * ULP * (1 + tmax)), final_error=abs(float(ref.mp.mpf(fs["final_error"]) - m["final_error"])),
                    final_hessian=dist(fs["final_hessian"].tolist(), m["final_hessian"]))


def judge_align(got, name):
    """got: summary_of / summary_from -> (passes, figures)."""
    m, fl = aligned(name, "mp"), align_floors(name)
    flags = ("iterations", "converged", "lm_failed", "n_correspondences")
    if any(got[k] != m[k] for k in flags):
        return False, {k: (got[k], m[k]) for k in flags}
    with ref.mp.workdps(ref.DPS):
        dist = lambda g, want: float(max(abs(ref.mp.mpf(float(x)) - w) for gr, wr in zip(g, want) for x, w in zip(gr, wr)))
        d = dict(T=dist(got["T"].tolist(), m["T"]), final_error=abs(float(ref.mp.mpf(got["final_error"]) - m["final_error"])),
                 final_hessian=dist(got["final_hessian"].tolist(), m["final_hessian"]))
    v = {k: (d[k], fl[k], d[k] <= ref.MARGIN * fl[k]) for k in d}
    return all(x[2] for x in v.values()), v
