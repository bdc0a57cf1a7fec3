"""Scan-to-map association of lidar_mapping restated from the reference's text (test infrastructure; numpy + mpmath, shares no code with
oracle/oracle_map.cpp or csrc/vilmap.hip and uses a different algorithm at every step).

  transform   pointAssociateToMap, localMapping.cpp:170-179: q * p + t in double (Eigen's quaternion-times-vector, three cross products -- not a rotation
              matrix), stored as float.  A query whose float rounding could differ between two float64 routes is flagged `xform_sensitive`.
  search      nearestKSearch :616 (k = 5), :695 (k = 10): exhaustive; squared distance (dx dx + dy dy) + dz dz with every operation rounded to float32
              (numpy float32), ordered by (distance, index); gate `pointSearchSqDis[4] < 1.0` :630, :713.  Beside it the five ways a compiler may
              contract that sum into one or two fused multiply-adds (FUSED), emulated in float64 -- the products of two float32 are exact there -- with
              one rounding per fused operation, and whether any of them changes what the fit is given (`sensitive`).
  corner      :632-667: centre and scatter matrix of the five in float64 as the reference forms them; eigen-decomposition of THAT matrix by mpmath.eigsy at
              50 digits (the judge) and by numpy.linalg.eigh (the float64 floor); gate eigenvalues[2] > 3 eigenvalues[1] :657; a, b = centre +- 0.1 u :661-662.
  surf        :697-709: re-rank the ten by float32 |intensity difference|, std::sort of (difference, index) pairs, keep five; :711-747: P n = -1 solved at 50
              digits through the normal equations (50 digits carry cond(P)^2) and by numpy.linalg.lstsq (the floor); d = 1 / |n|, n normalised, valid while
              no |n . p_j + d| > 0.2.
  rule-dependent   a P of numerical rank < 3 (smallest singular value <= 1e-12 largest, mpmath.svd_r): what colPivHouseholderQr().solve returns then hangs on
              Eigen's pivot threshold, which this file does not guess: the query is flagged and carries no expectation.

Decision floors (the issue's tau): corner 64 eps relative to lambda_2; surf 16 x the float64 floor of the residual of that query (never below half a unit in
the last place of the residual's largest term).  A query within tau of a gate is `decided = False`.

defect=...  deliberate mistakes for the sharpness checks of tests/test_mapreg_ref.py: "col1" (eigenvector column 1), "lam0" (gate lambda_2 > 3 lambda_0),
"norerank" (the five nearest instead of the five closest in intensity), "ge" (distance gate >= for <), "le" (<= for <).
"""
import functools
import types

import mpmath
import numpy as np

F32 = np.float32
EPS = 2.0 ** -52
TAU_CORNER = 64 * EPS
RANK_TOL = 1e-12
FUSED = ("fma_x", "fma_y", "fma_z", "fma_xz", "fma_yz")        # which product(s) ride in a fused multiply-add; "fma_x" = fma(dx, dx, dy dy) + dz dz, ...

mp = mpmath.mp.clone()
mp.dps = 50


# ---- transform ------------------------------------------------------------------------------------------------------------------------------------------
def transform(pts, q, t):
    """float32 [n, 3] of q * p + t (q = [x y z w]), and the flag of the points whose float rounding sits within 8 eps of a rounding boundary."""
    p = np.asarray(pts, np.float64)[:, :3]
    u, w = np.asarray(q, np.float64)[:3], float(q[3])
    uv = 2.0 * np.cross(u[None, :], p)
    pw = p + w * uv + np.cross(u[None, :], uv) + np.asarray(t, np.float64)[None, :]
    s = pw.astype(F32)
    mag = np.abs(p).sum(axis=1, keepdims=True) + np.abs(np.asarray(t, np.float64)).sum()
    wob = 8 * EPS * mag
    flag = np.any(((pw + wob).astype(F32) != s) | ((pw - wob).astype(F32) != s), axis=1)
    if not np.any(u):                                           # no rotation: p + t is one rounded addition by every route
        flag[:] = False
    return s, flag


# ---- search ---------------------------------------------------------------------------------------------------------------------------------------------
def _add_round32(a, b):
    """float32(a + b) of float64 arrays whose exact sum may not fit a float64: the float64 sum is nudged off a float32 rounding tie by the sign of its own
    rounding error (two-sum), so the second rounding cannot go the wrong way."""
    s = a + b
    bb = s - a
    err = (a - (s - bb)) + (b - bb)
    lo = s.astype(F32)
    back = lo.astype(np.float64)
    other = np.where(back <= s, np.nextafter(lo, F32(np.inf)), np.nextafter(lo, F32(-np.inf))).astype(np.float64)
    tie = (np.abs(s - back) == np.abs(other - s)) & (err != 0)
    s = np.where(tie, np.nextafter(s, np.where(err > 0, np.inf, -np.inf)), s)
    return s.astype(F32)


def sqdist(s, M, variant=None):
    """float32 squared distances of the float32 query s to the float32 points M [n, 3]: unfused (variant None) or one of FUSED."""
    d = (s[None, :].astype(F32) - M[:, :3].astype(F32)).astype(F32)
    if variant is None:
        return (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
    e = d.astype(np.float64)
    xx, yy, zz = e[:, 0] * e[:, 0], e[:, 1] * e[:, 1], e[:, 2] * e[:, 2]             # exact
    r32 = lambda v: v.astype(F32).astype(np.float64)
    if variant in ("fma_x", "fma_xz"):
        inner = _add_round32(xx, r32(yy))
    elif variant in ("fma_y", "fma_yz"):
        inner = _add_round32(r32(xx), yy)
    else:
        inner = _add_round32(r32(xx), r32(yy))
    inner = inner.astype(np.float64)
    return _add_round32(inner, zz if variant in ("fma_z", "fma_xz", "fma_yz") else r32(zz))


def knn(s, M, k, variant=None):
    d = sqdist(s, M, variant)
    order = np.lexsort((np.arange(len(d)), d))[:k]
    return order, d[order]


def rerank(nn, M, intensity):
    """:697-709: std::sort of (float |difference|, index) pairs, the first five"""
    diff = np.abs((M[nn, 3].astype(F32) - F32(intensity)).astype(F32))
    return [int(j) for _, j in sorted(zip(diff.tolist(), [int(j) for j in nn]))[:5]]


# ---- fits -----------------------------------------------------------------------------------------------------------------------------------------------
def scatter(P):
    """:633-649 in float64: centre = sum / 5, covMat = sum (p - centre)(p - centre)^T, in the reference's order"""
    P = np.asarray(P, np.float64)
    c = np.zeros(3)
    for p in P:
        c = c + p
    c = c / 5.0
    A = np.zeros((3, 3))
    for p in P:
        z = p - c
        A = A + np.outer(z, z)
    return c, A


def _f(v):
    return np.array([float(x) for x in v])


def corner_fit(P, defect=None):
    c, A = scatter(P)
    E, Q = mp.eigsy(mp.matrix(A.tolist()))                     # ascending
    order = sorted(range(3), key=lambda i: E[i])
    lam = [E[i] for i in order]
    col = order[1 if defect == "col1" else 2]
    u = [Q[r, col] for r in range(3)]
    l2, l1 = lam[2], lam[0 if defect == "lam0" else 1]
    ok = l2 > 3 * l1
    margin = float((l2 - 3 * l1) / l2) if l2 > 0 else -1.0      # an exactly zero scatter: 0 > 0 is false whatever the arithmetic
    tenth = mp.mpf(0.1)
    a = [tenth * u[r] + mp.mpf(c[r]) for r in range(3)]
    b = [-tenth * u[r] + mp.mpf(c[r]) for r in range(3)]
    w64, V64 = np.linalg.eigh(A)
    u64 = V64[:, 2]
    if float(sum(u64[r] * float(u[r]) for r in range(3))) < 0:
        u64 = -u64
    return types.SimpleNamespace(kind="corner", centre=c, A=A, lam=lam, lam64=w64, u=u, ok=bool(ok), margin=margin, tau=TAU_CORNER, decided=abs(margin) > TAU_CORNER,
                                 rule_dependent=False, a=a, b=b, value=np.concatenate([_f(a), _f(b)]), value64=np.concatenate([0.1 * u64 + c, -0.1 * u64 + c]),
                                 gap=float((lam[2] - lam[1]) / lam[2]) if l2 > 0 else 0.0)


def surf_fit(P):
    P = np.asarray(P, np.float64)
    Pm = mp.matrix(P.tolist())
    sv = sorted(mp.svd_r(Pm, compute_uv=False), reverse=True)
    out = types.SimpleNamespace(kind="surf", P=P, sv=[float(x) for x in sv], rule_dependent=bool(sv[2] <= RANK_TOL * sv[0]), ok=None, decided=False, margin=None, tau=None,
                                value=None, value64=None)
    if out.rule_dependent:
        return out
    n = mp.lu_solve(Pm.T * Pm, Pm.T * mp.matrix([-1] * 5))
    nn = mp.sqrt(sum(x * x for x in n))
    d = 1 / nn
    n = [x / nn for x in n]
    res = [abs(sum(n[r] * Pm[j, r] for r in range(3)) + d) for j in range(5)]
    n64 = np.linalg.lstsq(P, -np.ones(5), rcond=None)[0]
    nn64 = np.sqrt(n64 @ n64)
    d64 = 1.0 / nn64
    n64 = n64 / nn64
    res64 = np.abs(P @ n64 + d64)
    floor = max(max(abs(mp.mpf(res64[j]) - res[j]) for j in range(5)), mp.mpf(2.0 ** -53) * (abs(d) + max(abs(n[r] * Pm[j, r]) for j in range(5) for r in range(3))))
    out.tau = 16 * float(floor)
    out.margin = float(mp.mpf(0.2) - max(res))                  # 0.2: the double literal of :735
    out.ok = bool(max(res) <= mp.mpf(0.2))
    out.decided = abs(out.margin) > out.tau
    out.n, out.d = n, d
    out.value, out.value64 = _f(list(n) + [d]), np.concatenate([n64, [d64]])
    out.cond = out.sv[0] / out.sv[2]
    return out


# ---- association ----------------------------------------------------------------------------------------------------------------------------------------
def _gate(d5, defect):
    if defect == "ge":
        return bool(d5 >= F32(1.0))
    if defect == "le":
        return bool(d5 <= F32(1.0))
    return bool(d5 < F32(1.0))


def _query(i, s, xs, pt, M, k, surf, defect, with_fused):
    nn, d = knn(s, M, k)
    picks = lambda order: tuple(sorted(rerank(order, M, pt[3]))) if surf else tuple(sorted(int(j) for j in order))
    rec = types.SimpleNamespace(index=i, surf=surf, cp=np.asarray(pt[:3], np.float64), s=s, nn=nn, d=d, d5=d[4], gate=_gate(d[4], defect), xform_sensitive=bool(xs), fused={},
                                sensitive=False, list_sensitive=False, fit=None)
    if with_fused:
        for v in FUSED:
            vn, vd = knn(s, M, k, v)
            rec.fused[v] = (vn, vd, _gate(vd[4], defect))
            rec.list_sensitive |= bool(not np.array_equal(vn, nn) or rec.fused[v][2] != rec.gate)
            rec.sensitive |= bool(rec.fused[v][2] != rec.gate or (rec.gate and picks(vn) != picks(nn)))
    if rec.gate:
        if surf:
            rec.picks = nn[:5].tolist() if defect == "norerank" else rerank(nn, M, pt[3])
            rec.fit = surf_fit(M[rec.picks, :3])
        else:
            rec.picks = nn.tolist()
            rec.fit = corner_fit(M[nn, :3], defect)
    return rec


def associate(cmap, smap, sc, ss, q, t, defect=None, with_fused=True):
    """Every query's record, corner points then surf points, in scan order.  A class whose map holds fewer than k points yields nothing (nearestKSearch
    returns fewer than five / ten: index 4 of :630 / the ten of :706 do not exist)."""
    cmap, smap = np.asarray(cmap, F32).reshape(-1, 4), np.asarray(smap, F32).reshape(-1, 4)
    sc, ss = np.asarray(sc, F32).reshape(-1, 4), np.asarray(ss, F32).reshape(-1, 4)
    out = types.SimpleNamespace(corner=[], surf=[])
    for recs, scan, M, k, surf in ((out.corner, sc, cmap, 5, False), (out.surf, ss, smap, 10, True)):
        if len(M) < k or len(scan) == 0:
            continue
        s, xs = transform(scan, q, t)
        for i in range(len(scan)):
            recs.append(_query(i, s[i], xs[i], scan[i], M, k, surf, defect, with_fused))
    return out


def status(rec):
    """'accept' / 'reject' when the restatement decides the query, 'open' within tau of a gate or where the transform's rounding is open, 'rule' when rule-dependent"""
    if rec.xform_sensitive:
        return "open"
    if not rec.gate:
        return "reject"
    if rec.fit.rule_dependent:
        return "rule"
    if not rec.fit.decided:
        return "open"
    return "accept" if rec.fit.ok else "reject"


def tables(recs, use64=False):
    """The accepted factors in scan order: rows [cp, value] of the records `status` accepts"""
    rows = [np.concatenate([r.cp, r.fit.value64 if use64 else r.fit.value]) for r in recs if status(r) == "accept"]
    width = 7 if (recs and recs[0].surf) else 9
    return np.array(rows).reshape(-1, width)


def edge_distance(got, want):
    """per row max |a, b difference|, up to the swap the sign of u allows"""
    same = np.abs(got[:, 3:] - want[:, 3:]).max(axis=1)
    swap = np.maximum(np.abs(got[:, 3:6] - want[:, 6:9]).max(axis=1), np.abs(got[:, 6:9] - want[:, 3:6]).max(axis=1))
    return np.minimum(same, swap)


@functools.lru_cache(maxsize=None)
def cached(key):
    """associate() of a fixture of mapreg_fixtures by name (computed once per process, never modified)"""
    import mapreg_fixtures as mf
    fx = mf.get(key)
    return associate(fx.cmap, fx.smap, fx.sc, fx.ss, fx.q, fx.t)


# ---- judging an implementation's tables -------------------------------------------------------------------------------------------------------------------
MARGIN = 16.0                   # a device operation order over a float64 floor (tests/test_gpu_posegraph.py)
CLASSES = ("ab", "n", "d")


def _dist(cls, got, rec):
    """distance of one emitted row from the record's 50-digit values in one output class"""
    v = rec.fit.value
    if cls == "ab":
        return float(edge_distance(np.concatenate([np.zeros(3), got])[None, :], np.concatenate([np.zeros(3), v])[None, :])[0])
    return float(np.abs(got[:3] - v[:3]).max()) if cls == "n" else float(abs(got[3] - v[3]))


def floors(names, clamp=True):
    """per output class: the largest distance, over the accepted queries of the named fixtures, between the float64 route and the 50-digit values (a distance
    between float64 numbers is not resolved below half a unit in the last place of the value: a route that lands on the rounded 50-digit value counts as that).
    clamp=False: the measured distance alone -- what shows that the float64 route really differs from the 50-digit one."""
    out = dict.fromkeys(CLASSES, 0.0)
    for name in names:
        a = cached(name)
        for rec in a.corner + a.surf:
            if status(rec) == "accept":
                for cls in (("n", "d") if rec.surf else ("ab",)):
                    size = np.abs(rec.fit.value[3] if cls == "d" else rec.fit.value[:3] if cls == "n" else rec.fit.value).max()
                    out[cls] = max(out[cls], _dist(cls, rec.fit.value64, rec), 0.5 * float(np.spacing(size)) if clamp else 0.0)
    return out


def judge(assoc, edge, plane, floor=None):
    """An implementation's tables (vmap_associate layout) against the records of `assoc`.  Returns (problems, distances per class, {(surf, index): emitted} of the
    rule-dependent queries, number of open queries).  D1: a decided query must be present / absent as the restatement says; D2: its values within
    MARGIN x floor[class] (floor None: distances are only measured)."""
    problems, dist, rule, n_open = [], dict.fromkeys(CLASSES, 0.0), {}, 0
    for recs, got, surf in ((assoc.corner, np.asarray(edge), False), (assoc.surf, np.asarray(plane), True)):
        ptr = 0
        for rec in recs:
            present = ptr < len(got) and np.array_equal(got[ptr, :3], rec.cp)
            row = got[ptr, 3:] if present else None
            ptr += int(present)
            st = status(rec)
            if st == "open":
                n_open += 1
            elif st == "rule":
                rule[(surf, rec.index)] = present
                if present and not (np.all(np.isfinite(row)) and abs(np.linalg.norm(row[:3]) - 1.0) < 1e-12):
                    problems.append(("rule-dependent row not finite / not unit", surf, rec.index))
            elif (st == "accept") != present:
                problems.append(("accepted" if present else "missing", surf, rec.index))
            elif present:
                for cls in (("n", "d") if surf else ("ab",)):
                    e = _dist(cls, row, rec)
                    dist[cls] = max(dist[cls], e)
                    if floor is not None and not e <= MARGIN * floor[cls]:
                        problems.append((cls, surf, rec.index, e, floor[cls]))
        if ptr != len(got):
            problems.append(("rows that belong to no query, or out of scan order", surf, len(got) - ptr))
    return problems, dist, rule, n_open


# ---- the first trust-region step of vmap_align (localMapping.cpp:596-600, :766-777; the algorithm of tests/step_ref.py on one pose block) ----------------
# vmap_align runs two rounds of {associate, solve} and hands back only the pose after the second; with max_iterations = 1 each round is ONE dogleg step from a
# fresh trust-region state (Jacobi scales, radius, mu are re-made per round).  The reference route is therefore applied twice: round one from the fixture's
# pose on the restatement's factors there, round two from the pose round one ends in, on the restatement's factors THERE.  The float64 route is applied twice
# the same way (its own pose between the rounds, its own float64 factor values), and both end poses are read back as a step from the 50-digit route's
# intermediate pose -- so whatever error a float64 implementation carries from round one into round two is in the floor, not in an allowance made up here.
_LD = np.longdouble


def _one_pose_state(pose7):
    """a pose [t, q] as the state image step_ref.read_step / read_noise take: a window of one pose, nothing else moving"""
    return {"pose": np.asarray(pose7, np.float64).reshape(1, 7), "speedbias": np.zeros((1, 9)), "ex_pose": np.array([0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 1.0]),
            "td": np.zeros(1), "inv_depth": np.zeros(0)}


ONE_POSE = types.SimpleNamespace(K=1, D=22, L=0)


def linearise(S, edge, plane, pose7):
    """[(residual, Jacobian over the six tangent coordinates)] of the edge / plane rows at pose7, in the arithmetic S of factors_ref (dual numbers), float64 or
    50 digits; identity extrinsic"""
    import factors_ref as fr
    out = []
    for kind, rows in ((2, plane), (0, edge)):
        for row in rows:
            cols = []
            for k in range(6):
                P, Q = fr.pose_tangent(S, pose7, k)
                r, _ = fr.lidar_residual(S, kind, list(row), [0.0, 0.0, 0.0, 1.0], [0.0, 0.0, 0.0], P, Q)
                cols.append([fr.der(x, S) for x in r])
            out.append(([fr.val(x) for x in r], [[cols[k][i] for k in range(6)] for i in range(len(r))]))
    return out


def normal_equations(lin, dtype, a=0.1):
    """H = sum rho' J^T J, g = sum rho' J^T r with HuberLoss(a) (rho' = 1 for |r| <= a, a / |r| above; ceres' corrector with rho'' <= 0 is this scaling)"""
    to = (lambda x: _LD(mpmath.nstr(x, 30))) if dtype is _LD else float
    H, g = np.zeros((6, 6), dtype), np.zeros(6, dtype)
    for r, J in lin:
        r = np.array([to(x) for x in r], dtype)
        J = np.array([[to(x) for x in row] for row in J], dtype)
        n = np.sqrt(r @ r)
        w = dtype(1) if n <= dtype(a) else dtype(a) / n
        H += w * (J.T @ J)
        g += w * (J.T @ r)
    return H, g


def plus(pose7, step, dtype):
    """pose_local_parameterization.cpp:3-18: p + dp, q (x) [dtheta / 2, 1] normalised; evaluated in dtype, stored as float64"""
    p, d = np.asarray(pose7).astype(dtype), np.asarray(step).astype(dtype)
    x, y, z, w = p[3:]
    a, b, c = d[3:] * dtype(0.5)
    q = np.array([w * a + x + (y * c - z * b), w * b + y + (z * a - x * c), w * c + z + (x * b - y * a), w - (x * a + y * b + z * c)], dtype)
    q = q / np.sqrt(q @ q)
    return np.concatenate([p[:3] + d[:3], q]).astype(np.float64)


@functools.lru_cache(maxsize=None)
def two_rounds(radius, jacobi=1, mu=1e-8):
    """Both routes through two one-iteration rounds on the random fixture at initial_radius `radius`."""
    import factors_ref as fr
    import mapreg_fixtures as mf
    import step_ref as sr
    fx = mf.get("random")
    out = types.SimpleNamespace(radius=radius, rounds=[])
    pose_ld = pose_64 = np.concatenate([fx.t, fx.q])
    for rnd in range(2):
        assoc = cached("random") if rnd == 0 else associate(fx.cmap, fx.smap, fx.sc, fx.ss, pose_ld[3:], pose_ld[:3], with_fused=False)
        undecided = [r.index for r in assoc.corner + assoc.surf if status(r) in ("open", "rule")]
        Hl, gl = normal_equations(linearise(fr.MP, tables(assoc.corner), tables(assoc.surf), [float(v) for v in pose_ld]), _LD)
        H6, g6 = normal_equations(linearise(fr.F64, tables(assoc.corner, use64=True), tables(assoc.surf, use64=True), [float(v) for v in pose_64]), np.float64)
        ld, f64 = sr.Route(Hl, gl, jacobi, mu, _LD), sr.Route(H6, g6, jacobi, mu, np.float64)
        (br_ld, y_ld), (br_64, y_64) = ld.dogleg(radius), f64.dogleg(radius)
        same = f64                                  # the float64 route from the SAME start: the float64 LU "on the same system" that omega_64 belongs to
        if rnd:
            same = sr.Route(*normal_equations(linearise(fr.F64, tables(assoc.corner, use64=True), tables(assoc.surf, use64=True), [float(v) for v in pose_ld]), np.float64),
                            jacobi, mu, np.float64)
        out.rounds.append(types.SimpleNamespace(start=pose_ld, start64=pose_64, ld=ld, f64=f64, branch=br_ld, branch64=br_64, y=y_ld, y64=y_64, undecided=undecided,
                                                n_edge=len(tables(assoc.corner)), n_plane=len(tables(assoc.surf)),
                                                omega64=sr.omega(ld.M, ld.rhs, same.x), omega_ref=sr.omega(ld.M, ld.rhs, ld.x)))
        pose_ld, pose_64 = plus(pose_ld, ld.s * y_ld, _LD), plus(pose_64, f64.s * y_64, np.float64)
    out.end, out.end64 = pose_ld, pose_64
    return out


def check_two_rounds(ref, pose2, tag):
    """An implementation's pose after two one-iteration rounds against two_rounds(): read as the step of round two from the 50-digit route's intermediate pose.

    forward (every branch; the assertion of step_ref.check_step's Cauchy / interpolated branches): per scaled component
        |y - y_ld| <= MARGIN max|y_64 - y_ld| + 2 noise,
      y_64 the float64 route's end pose read the same way, noise = step_ref.read_noise (2^-52 |t|, 2^-50 per rotation component), twice because the
      implementation stores a rounded pose after each round and round two adds to the stored one.
    backward (Gauss-Newton branch): x = -y solves M x = rhs of round two with the Oettli-Prager error
        omega <= MARGIN omega_64 + max_i (|M| 2 noise)_i / (|M| |x| + |rhs|)_i.
      omega_64 is that of the float64 LU on the same system (step_ref.MARGIN = 20 over it, as tests/test_gpu_step.py).  The second term: the pose read back is
      x + e with |e| <= 2 noise, so |rhs - M (x + e)| <= |rhs - M x| + |M| |e|.  What round one's own error delta leaves in this residual is smaller still: the
      implementation solves round two at start + delta, where rhs' = rhs + s H delta, and the step read from `start` is x' - delta / s, so
      M (x' - delta / s) = rhs - mu d^2 delta / s + O(delta |x|): the Gauss-Newton step lands on the same point from either start (mu = 1e-8).
    Returns the figures."""
    import step_ref as sr
    r2 = ref.rounds[1]
    s2 = np.asarray(r2.ld.s, np.float64)
    before = _one_pose_state(r2.start)
    y = sr.read_step(ONE_POSE, before, _one_pose_state(pose2))[:6] / s2
    y64 = sr.read_step(ONE_POSE, before, _one_pose_state(ref.end64))[:6] / s2
    noise = 2.0 * sr.read_noise(ONE_POSE, before, np.concatenate([s2, np.ones(16)]))[:6]
    err = np.abs(y.astype(_LD) - r2.y)
    err64 = float(np.abs(y64.astype(_LD) - r2.y).max())
    size = float(np.abs(r2.y).max())
    fig = types.SimpleNamespace(branch=r2.branch, forward=float(err.max()) / size, forward64=err64 / size, noise=float(noise.max()) / size, omega=None)
    line = "%s radius %g rounds %s/%s: forward error %.3e (float64 route %.3e, read noise %.3e) of max|step / s| = %.3e" % (
        tag, ref.radius, ref.rounds[0].branch, r2.branch, fig.forward, fig.forward64, fig.noise, size)
    ok_forward = bool(np.all(err <= sr.MARGIN * err64 + noise))
    ok_backward = True
    if r2.branch == sr.GN:
        M, rhs, x = np.asarray(r2.ld.M, _LD), np.asarray(r2.ld.rhs, _LD), -y.astype(_LD)
        fig.omega = sr.omega(M, rhs, x)
        fig.omega_noise = float(((np.abs(M) @ noise.astype(_LD)) / (np.abs(M) @ np.abs(x) + np.abs(rhs))).max())
        fig.omega64 = r2.omega64
        ok_backward = fig.omega <= sr.MARGIN * r2.omega64 + fig.omega_noise
        line += "; omega %.3e (float64 LU %.3e, read noise carried %.3e)" % (fig.omega, r2.omega64, fig.omega_noise)
    print(line)
    assert ok_forward and ok_backward, line
    return fig
