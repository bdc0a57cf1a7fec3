"""Test infrastructure: a restatement of the voxelised GICP registration of include/vilvgicp.h, written from fast_gicp's statements
(gicp/impl/fast_vgicp_impl.hpp:73-204, gicp/impl/lsq_registration_impl.hpp:48-165, gicp/impl/fast_gicp_impl.hpp:241-300, so3/so3.hpp:53-77,
gicp/fast_vgicp_voxel.hpp:10-44 and :161-163).  It shares no code with oracle/ or csrc/.

Generic over its arithmetic: F64 (Python floats = IEEE doubles, numpy for the general solves) and MP (mpmath at 50 digits).  Everything is
written on nested lists of scalars, so the two routes run the same statements.

What is NOT generic is the contract itself:
  * voxel_coord is floor(x / res - 0.5) in IEEE double, of the transformed point computed in double;
  * the neighbours of the covariance estimate are the k smallest by (float32 squared distance, index), the distance
    fl(fl(fl(dx*dx) + fl(dy*dy)) + fl(dz*dz)) with every rounding to float32 and nothing fused.
Both routes take the correspondences / neighbours from those, so they differ only in the rounding of the arithmetic that follows.

The judge (MARGIN = 16, as mapreg_ref): floor = the largest distance of the float64 route from the 50-digit values, per quantity; an
implementation passes when its own distance is at most MARGIN x floor.  The float64 route inverts by adjugate and 1 / determinant (Eigen's
fixed-size inverse) and adds the correspondences one after the other.  The reference adds them under an OpenMP reduction, in no fixed order,
so the route is evaluated twice, in ascending and in descending slot order (F64_ROUTES), and the floor is the larger distance.  One order
alone is no floor: on 15 of the 270 DIRECT1 / DIRECT7 edge cases the descending sum is more than 16 x the ascending sum's distance from the
50-digit error (and on 8 the other way round), because one realisation of the roundings can land within a few hundredths of an ulp of the
exact value (docs/vgicp.md has the figures)."""
import functools
import math

import mpmath as mp
import numpy as np

import voxelmap_ref as vr

F = np.float32
DPS = 50
MARGIN = 16.0
DIRECT1, DIRECT7, DIRECT27 = 1, 7, 27
LM, GN = 0, 1
QUANTITIES = ("err", "b_rot", "b_trans", "H_rr", "H_rt", "H_tt")


def at50(fn):
    @functools.wraps(fn)
    def run(*a, **k):
        with mp.workdps(DPS):
            return fn(*a, **k)
    return run


# ---- the two arithmetics ----------------------------------------------------------------------------------------------------------
class F64:
    name = "f64"
    num = staticmethod(float)
    sqrt, sin, cos = staticmethod(math.sqrt), staticmethod(math.sin), staticmethod(math.cos)

    @staticmethod
    def inv3(a):
        """Adjugate and 1 / determinant (what Eigen does for fixed sizes up to 4)."""
        c = [[a[(i + 1) % 3][(j + 1) % 3] * a[(i + 2) % 3][(j + 2) % 3] - a[(i + 1) % 3][(j + 2) % 3] * a[(i + 2) % 3][(j + 1) % 3] for j in range(3)] for i in range(3)]
        det = a[0][0] * c[0][0] + a[0][1] * c[0][1] + a[0][2] * c[0][2]
        inv = 1.0 / det
        return [[c[j][i] * inv for j in range(3)] for i in range(3)]

    @staticmethod
    def solve(A, b):
        return [float(v) for v in np.linalg.solve(np.array(A, np.float64), np.array(b, np.float64))]

    @staticmethod
    def eigh(A):
        w, V = np.linalg.eigh(np.array(A, np.float64))
        return [float(v) for v in w], [[float(V[r][c]) for c in range(3)] for r in range(3)]


class MP:
    name = "mp"
    num = staticmethod(lambda x: mp.mpf(float(x)) if not isinstance(x, mp.mpf) else x)
    sqrt, sin, cos = staticmethod(mp.sqrt), staticmethod(mp.sin), staticmethod(mp.cos)

    @staticmethod
    def inv3(a):
        m = mp.matrix(a) ** -1
        return [[m[i, j] for j in range(3)] for i in range(3)]

    @staticmethod
    def solve(A, b):
        x = mp.lu_solve(mp.matrix(A), mp.matrix(b))
        return [x[i] for i in range(len(b))]

    @staticmethod
    def eigh(A):
        w, V = mp.eigsy(mp.matrix(A))
        order = sorted(range(3), key=lambda i: w[i])
        return [w[i] for i in order], [[V[r, c] for c in order] for r in range(3)]


def mat(A, T):
    return [[A.num(v) for v in row] for row in np.asarray(T, np.float64).tolist()]


# ---- voxel coordinate, offsets ----------------------------------------------------------------------------------------------------
@at50
def voxel_coord(x, res):
    """(floor(x / res - 0.5) in IEEE double, the 50-digit distance of q = x / res - 0.5 from the nearest integer, |q|).  x: a double or an
    mpf; the floor is taken of float(x)."""
    xd, rd = float(x), float(res)
    q = mp.mpf(x) / mp.mpf(rd) - mp.mpf(0.5)
    return int(math.floor(xd / rd - 0.5)), abs(q - mp.nint(q)), abs(q)


def offsets(mode):
    """neighbor_offsets (fast_vgicp_voxel.hpp:10-44) as a set of integer triples."""
    if mode == DIRECT1:
        return frozenset({(0, 0, 0)})
    if mode == DIRECT7:
        return frozenset({(0, 0, 0), (1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1)})
    if mode == DIRECT27:
        return frozenset((i - 1, j - 1, k - 1) for i in range(3) for j in range(3) for k in range(3))
    raise ValueError(mode)


# ---- a registration problem -------------------------------------------------------------------------------------------------------
class Problem:
    """Target cloud + covariances -> voxelmap_ref.build (the byte-exact contract of the map); source cloud + covariances."""

    def __init__(self, tx, tc, sx, sc, res):
        self.tx = np.ascontiguousarray(tx, F).reshape(-1, 3); self.tc = np.ascontiguousarray(tc, np.float64).reshape(-1, 9)
        self.sx = np.ascontiguousarray(sx, F).reshape(-1, 3); self.sc = np.ascontiguousarray(sc, np.float64).reshape(-1, 9)
        self.res = float(res)
        self.map = vr.build(self.tx, self.tc, self.res)
        number = {int(k): v for v, k in enumerate(self.map["keys"])}
        # looked up by the integer triple itself, as the reference's unordered_map of Eigen::Vector3i: nothing aliases
        self.lookup = {}
        for c in vr.voxel_coords(self.tx, self.res):
            t = tuple(int(v) for v in c)
            assert all(-(1 << 20) <= v < (1 << 20) for v in t), "target voxel outside the 21-bit key"
            self.lookup[t] = number[vr.pack_key(*t)]
        self._corr = {}

    def correspondences(self, T, mode, coord=None, offs=None):
        """Per slot (source-major, the offsets in sorted order): the voxel number or None; per source point: open or not.
        coord: a replacement for voxel_coord's integer, offs: a replacement for offsets(mode) (the mutants)."""
        T = np.ascontiguousarray(T, np.float64)
        key = (T.tobytes(), coord)
        if key not in self._corr:
            self._corr[key] = self._coords(T, coord)
        coords, opened = self._corr[key]
        offs = sorted(offsets(mode) if offs is None else offs)
        vox = [self.lookup.get((c[0] + o[0], c[1] + o[1], c[2] + o[2])) for c in coords for o in offs]
        return vox, opened, len(offs)

    @at50
    def _coords(self, T, coord):
        Tl = T.tolist(); Tm = mat(MP, T)
        coords, opened = [], []
        for a in self.sx.astype(np.float64).tolist():
            c, is_open = [], False
            for r in range(3):
                x = Tl[r][0] * a[0] + Tl[r][1] * a[1] + Tl[r][2] * a[2] + Tl[r][3]                 # Eigen: trans * mean_A in double
                xe = Tm[r][0] * MP.num(a[0]) + Tm[r][1] * MP.num(a[1]) + Tm[r][2] * MP.num(a[2]) + Tm[r][3]
                k, _, _ = voxel_coord(x, self.res)
                _, dist, aq = voxel_coord(xe, self.res)
                if xe != mp.mpf(x) and dist <= mp.mpf(1e-12) * (aq + 1):
                    is_open = True
                c.append(k if coord is None else coord(x, self.res))
            coords.append(c); opened.append(is_open)
        return coords, opened


def _mahalanobis(A, P, T, i, v, rcr_R=None):
    """M = (cov_B + R cov_A R^T)^-1 of one correspondence."""
    Rc = [row[:3] for row in T] if rcr_R is None else rcr_R
    ca = [[A.num(P.sc[i][3 * r + c]) for c in range(3)] for r in range(3)]
    cb = [[A.num(P.map["cov"][v][3 * r + c]) for c in range(3)] for r in range(3)]
    RC = [[sum(Rc[r][k] * ca[k][c] for k in range(3)) for c in range(3)] for r in range(3)]
    RCR = [[cb[r][c] + sum(RC[r][k] * Rc[c][k] for k in range(3)) for c in range(3)] for r in range(3)]
    return A.inv3(RCR)


def _fold(terms, order, zero):
    """The sum of the per-slot term vectors, one after the other from zero, in ascending ('asc') or descending ('desc') slot order."""
    if not terms:
        return None
    acc = [zero] * len(terms[0])
    for t in (reversed(terms) if order == "desc" else terms):
        acc = [x + y for x, y in zip(acc, t)]
    return acc


def _accumulate(A, P, T, vox, Ms, noff, want_H, w_of, skew_sign, order="asc"):
    zero = A.num(0.0)
    R = [row[:3] for row in T]
    terms = []                                               # per correspondence: err | 21 H (upper) | 6 b
    for s, v in enumerate(vox):
        if v is None:
            continue
        M = Ms[s]
        a = [A.num(x) for x in P.sx[s // noff].astype(np.float64).tolist()]
        ta = [R[r][0] * a[0] + R[r][1] * a[1] + R[r][2] * a[2] + T[r][3] for r in range(3)]
        e = [A.num(P.map["mean"][v][r]) - ta[r] for r in range(3)]
        w = w_of(A, int(P.map["num"][v]))
        Me = [M[r][0] * e[0] + M[r][1] * e[1] + M[r][2] * e[2] for r in range(3)]
        term = [w * (e[0] * Me[0] + e[1] * Me[1] + e[2] * Me[2])]
        if want_H:
            sk = [[zero, -ta[2], ta[1]], [ta[2], zero, -ta[0]], [-ta[1], ta[0], zero]]                # skewd(transed_mean_A)
            J = [[skew_sign * sk[r][c] for c in range(3)] + [A.num(-1.0) if c == r else zero for c in range(3)] for r in range(3)]
            MJ = [[M[r][0] * J[0][q] + M[r][1] * J[1][q] + M[r][2] * J[2][q] for q in range(6)] for r in range(3)]
            term += [w * (J[0][p] * MJ[0][q] + J[1][p] * MJ[1][q] + J[2][p] * MJ[2][q]) for p in range(6) for q in range(p, 6)]
            term += [w * (J[0][p] * Me[0] + J[1][p] * Me[1] + J[2][p] * Me[2]) for p in range(6)]
        terms.append(term)
    H, b = [[zero] * 6 for _ in range(6)], [zero] * 6
    tot = _fold(terms, order, zero)
    if tot is None:
        return zero, H, b, 0
    if want_H:
        idx = 1
        for p in range(6):
            for q in range(p, 6):
                H[p][q] = H[q][p] = tot[idx]; idx += 1
        b = tot[22:28]
    return tot[0], H, b, len(terms)


def _w_sqrt(A, num):
    return A.sqrt(A.num(float(num)))


@at50
def linearize(P, T, mode, A, want_H=True, coord=None, offs=None, w_of=_w_sqrt, rcr_identity=False, skew_sign=1, order="asc", Ta=None):
    """FastVGICP::update_correspondences + linearize.  T: the transform in double (the correspondences are its contract); Ta: the same
    transform in the arithmetic when it carries more digits (the 50-digit loop's state).  Returns dict(err, H, b, n, vox, M, open, noff)."""
    T = np.ascontiguousarray(T, np.float64)
    vox, opened, noff = P.correspondences(T, mode, coord, offs)
    eye = [[A.num(1.0 if r == c else 0.0) for c in range(3)] for r in range(3)]
    if Ta is None:                                         # a pure function of (R, cov_A, voxel): computed once (the edge fixtures repeat it 129 times)
        Ta = mat(A, T)
        memo = P._corr.setdefault(("M", A.name, T[:3, :3].tobytes(), rcr_identity), {})

        def M_of(s, v):
            key = (P.sc[s // noff].tobytes(), v)
            if key not in memo:
                memo[key] = _mahalanobis(A, P, Ta, s // noff, v, eye if rcr_identity else None)
            return memo[key]
    else:
        M_of = lambda s, v: _mahalanobis(A, P, Ta, s // noff, v, eye if rcr_identity else None)
    Ms = [None if v is None else M_of(s, v) for s, v in enumerate(vox)]
    err, H, b, n = _accumulate(A, P, Ta, vox, Ms, noff, want_H, w_of, skew_sign, order)
    return dict(err=err, H=H, b=b, n=n, vox=vox, M=Ms, open=opened, noff=noff)


@at50
def compute_error(P, T2, lin, A, order="asc", Ta=None):
    """FastVGICP::compute_error: the correspondences and M of an earlier linearisation (of the same arithmetic), a new transform."""
    return _accumulate(A, P, mat(A, T2) if Ta is None else Ta, lin["vox"], lin["M"], lin["noff"], False, _w_sqrt, 1, order)[0]


def to_np(x):
    return np.array([[float(v) for v in row] for row in x]) if isinstance(x[0], list) else np.array([float(v) for v in x])


# ---- the judge ----------------------------------------------------------------------------------------------------------------------
def _parts(err, H, b):
    """The six quantities as flat lists."""
    out = {"err": [err]}
    if H is not None:
        out.update(b_rot=list(b[:3]), b_trans=list(b[3:]), H_rr=[H[p][q] for p in range(3) for q in range(3)],
                   H_rt=[H[p][q] for p in range(3) for q in range(3, 6)] + [H[p][q] for p in range(3, 6) for q in range(3)], H_tt=[H[p][q] for p in range(3, 6) for q in range(3, 6)])
    return out


@at50
def distance(got, ref):
    """Largest absolute distance per quantity of (err, H, b) in any number type from the 50-digit (err, H, b)."""
    g, r = _parts(*got), _parts(*ref)
    return {q: float(max(abs(mp.mpf(float(x)) - y) for x, y in zip(g[q], r[q]))) for q in g}


F64_ROUTES = ((F64, "asc"), (F64, "desc"))


def lin_floor(P, T, mode, ref, want_H=True):
    """The float64 floor of a linearisation, per quantity, against the 50-digit `ref`."""
    fl = {}
    for A, order in F64_ROUTES:
        l = linearize(P, T, mode, A, want_H, order=order)
        assert l["n"] == ref["n"]
        for q, d in distance((l["err"], l["H"] if want_H else None, l["b"]), (ref["err"], ref["H"] if want_H else None, ref["b"])).items():
            fl[q] = max(fl.get(q, 0.0), d)
    return fl


def verdict(dist, floor):
    """{quantity: (distance, floor, ok)}; ok: distance <= MARGIN x floor."""
    return {q: (dist[q], floor[q], dist[q] <= MARGIN * floor[q]) for q in dist}


# ---- covariances ------------------------------------------------------------------------------------------------------------------
def sqdist32(q, X, fuse=None):
    """fl(fl(fl(dx*dx) + fl(dy*dy)) + fl(dz*dz)), float32, unfused.  fuse: 'second' (fl(dx*dx + dy*dy_exact)), 'third' or 'both' -- the three
    contracted forms, emulated in float64 (a product of two float32 is exact in double) with one rounding to float32 per fused operation."""
    X = np.asarray(X, F); q = np.asarray(q, F)
    d = (q[None, :] - X).astype(F)
    dx, dy, dz = d[:, 0], d[:, 1], d[:, 2]
    if fuse is None:
        return ((dx * dx).astype(F) + (dy * dy).astype(F)).astype(F) + (dz * dz).astype(F)
    x2, y2, z2 = dx.astype(np.float64) ** 2, dy.astype(np.float64) ** 2, dz.astype(np.float64) ** 2     # exact
    if fuse == "second":                                    # fma(dy, dy, fl(dx*dx)), then + fl(dz*dz)
        s = (x2.astype(F).astype(np.float64) + y2).astype(F)
        return (s + z2.astype(F)).astype(F)
    if fuse == "third":                                     # fma(dz, dz, fl(fl(dx*dx) + fl(dy*dy)))
        s = (x2.astype(F) + y2.astype(F)).astype(F)
        return (s.astype(np.float64) + z2).astype(F)
    if fuse == "both":
        s = (x2.astype(F).astype(np.float64) + y2).astype(F)
        return (s.astype(np.float64) + z2).astype(F)
    raise ValueError(fuse)


def neighbours(xyz, i, k, fuse=None, larger_index_first=False):
    d = sqdist32(xyz[i], xyz, fuse)
    idx = np.arange(len(xyz))
    return np.lexsort((-idx if larger_index_first else idx, d))[:k]


@at50
def covariances(xyz, k, A, fuse=None, larger_index_first=False, largest=False, divisor=None, points=None):
    """FastGICP::calculate_covariances with RegularizationMethod::PLANE.  Returns (C (n, 3, 3) nested lists, relative gaps (l2 - l1) / l3).
    Only n >= k has expected values."""
    xyz = np.ascontiguousarray(xyz, F).reshape(-1, 3)
    assert len(xyz) >= k
    div = A.num(float(k if divisor is None else divisor))                  # (the mutant divides the mean and the covariance by k - 1)
    out, gaps = [], []
    for i in (range(len(xyz)) if points is None else points):
        nb = [[A.num(v) for v in xyz[j].astype(np.float64).tolist()] for j in neighbours(xyz, i, k, fuse, larger_index_first)]
        mean = [sum((p[r] for p in nb), A.num(0.0)) / div for r in range(3)]
        C = [[sum(((p[r] - mean[r]) * (p[c] - mean[c]) for p in nb), A.num(0.0)) / div for c in range(3)] for r in range(3)]
        w, V = A.eigh(C)
        m = 2 if largest else 0
        n = [V[r][m] for r in range(3)]
        nn = A.sqrt(n[0] * n[0] + n[1] * n[1] + n[2] * n[2])
        n = [v / nn for v in n]
        f = A.num(1.0 - 1e-3)
        out.append([[A.num(1.0 if r == c else 0.0) - f * n[r] * n[c] for c in range(3)] for r in range(3)])
        gaps.append(float((w[1] - w[0]) / w[2]) if w[2] > 0 else 0.0)
    return out, gaps


@at50
def cov_distance(got, ref):
    """Per point: the largest absolute distance of a 3 x 3 from the 50-digit one."""
    return [float(max(abs(mp.mpf(float(g[r][c])) - C[r][c]) for r in range(3) for c in range(3))) for g, C in zip(got, ref)]


# ---- the optimiser ----------------------------------------------------------------------------------------------------------------
def so3_exp(A, w):
    """so3.hpp:53-77: the quaternion (w, x, y, z)."""
    t2 = w[0] * w[0] + w[1] * w[1] + w[2] * w[2]
    if t2 < 1e-10:
        t4 = t2 * t2
        im = A.num(0.5) - A.num(1.0) / A.num(48.0) * t2 + A.num(1.0) / A.num(3840.0) * t4
        re = A.num(1.0) - A.num(1.0) / A.num(8.0) * t2 + A.num(1.0) / A.num(384.0) * t4
    else:
        t = A.sqrt(t2); h = A.num(0.5) * t
        im = A.sin(h) / t; re = A.cos(h)
    return re, im * w[0], im * w[1], im * w[2]


def quat_matrix(A, q):
    """Eigen's Quaternion::toRotationMatrix (no normalisation)."""
    w, x, y, z = q
    one, two = A.num(1.0), A.num(2.0)
    return [[one - two * (y * y + z * z), two * (x * y - w * z), two * (x * z + w * y)],
            [two * (x * y + w * z), one - two * (x * x + z * z), two * (y * z - w * x)],
            [two * (x * z - w * y), two * (y * z + w * x), one - two * (x * x + y * y)]]


def _delta(A, d):
    return quat_matrix(A, so3_exp(A, d[:3])), list(d[3:])


def _times(A, Rd, td, x0):
    """delta * x0 for two isometries."""
    out = [[sum(Rd[r][k] * x0[k][c] for k in range(3)) for c in range(4)] for r in range(3)]
    for r in range(3):
        out[r][3] = out[r][3] + td[r]
    return out + [[A.num(0.0), A.num(0.0), A.num(0.0), A.num(1.0)]]


def _pivots(A, Hm):
    """The pivots of elimination without exchanges (the D of L D L^T for a symmetric matrix)."""
    a = [row[:] for row in Hm]
    piv = []
    for j in range(6):
        piv.append(a[j][j])
        for i in range(j + 1, 6):
            f = a[i][j] / a[j][j]
            for c in range(j, 6):
                a[i][c] = a[i][c] - f * a[j][c]
    return piv


@at50
def align(P, guess, opts, A, never_reject=False, lambda_without_cube=False):
    """LsqRegistration::computeTransformation with step_lm / step_gn / is_converged.  opts: dict(neighbor_mode, optimizer, max_iterations,
    lm_max_iterations, rotation_epsilon, transformation_epsilon, lm_init_lambda_factor).  Returns a dict with what vgicp_summary holds, T, the
    decisions taken (a tuple), the margins of those decisions, whether any iterate had an open slot, and the last linearisation used."""
    mode, reps, teps = opts["neighbor_mode"], A.num(opts["rotation_epsilon"]), A.num(opts["transformation_epsilon"])
    x0 = mat(A, guess)
    lam = A.num(-1.0)
    converged = False
    decisions, margins = [], dict(rho=[], conv=[], pivot=[])
    out = dict(iterations=0, converged=0, lm_failed=0, n_correspondences=0, final_error=A.num(0.0), any_open=False, lin=None,
               final_hessian=[[A.num(1.0 if r == c else 0.0) for c in range(6)] for r in range(6)])

    def is_converged(Rd, td):
        m = max(max(abs(Rd[r][c] - A.num(1.0 if r == c else 0.0)) for r in range(3) for c in range(3)) / reps, max(abs(v) for v in td) / teps)
        margins["conv"].append(float(abs(1 - m)))
        decisions.append(("conv", bool(m < 1)))
        return bool(m < 1)

    def linearise(x):
        l = linearize(P, to_np(x), mode, A, Ta=x)
        out["n_correspondences"], out["final_error"], out["lin"] = l["n"], l["err"], l
        out["any_open"] = out["any_open"] or any(l["open"])
        return l

    nr = -1
    for i in range(opts["max_iterations"]):
        if converged:
            break
        nr = i
        l = linearise(x0)
        H, b, y0 = l["H"], l["b"], l["err"]
        nb = [-v for v in b]
        if opts["optimizer"] == GN:                                                  # step_gn
            margins["pivot"].append(float(min(_pivots(A, H))))
            d = A.solve(H, nb)
            Rd, td = _delta(A, d)
            x0 = _times(A, Rd, td, x0)
            out["final_hessian"] = H
        else:                                                                        # step_lm
            if lam < 0:
                lam = A.num(opts["lm_init_lambda_factor"]) * max(abs(H[k][k]) for k in range(6))
            nu = A.num(2.0)
            stepped = False
            for _ in range(opts["lm_max_iterations"]):
                Hl = [[H[r][c] + (lam if r == c else 0) for c in range(6)] for r in range(6)]
                margins["pivot"].append(float(min(_pivots(A, Hl))))
                d = A.solve(Hl, nb)
                Rd, td = _delta(A, d)
                xi = _times(A, Rd, td, x0)
                yi = compute_error(P, None, l, A, Ta=xi)
                rho = (y0 - yi) / sum(d[k] * (lam * d[k] - b[k]) for k in range(6))
                margins["rho"].append(float(abs(rho)))
                reject = bool(rho < 0) and not never_reject
                decisions.append(("reject", bool(reject)))
                if reject:
                    if is_converged(Rd, td):
                        stepped = True
                        break
                    lam = nu * lam; nu = 2 * nu
                    continue
                x0 = xi
                c = 2 * rho - 1
                lam = lam * max(A.num(1.0) / A.num(3.0), 1 - (c if lambda_without_cube else c * c * c))
                out["final_hessian"] = H
                stepped = True
                break
            if not stepped:
                out["lm_failed"] = 1                                                 # "lm not converged!!"
                break
        converged = is_converged(Rd, td)
    out.update(iterations=nr + 1, converged=int(converged), T=x0, decisions=tuple(decisions), margins=margins)
    return out
