"""Synthetic pose graphs for the vpgo_* tests: a planar loop of radius 20 m with out-of-plane wobble, odometry noise 0.002 rad / 0.02 m,
odometry variances 0.05, the prior variances of globalMappingIkdTree.cpp:154, fixed seeds.  Generated, not stored.

A fixture is a dict: truth (N x 4 x 4), init (the drifted odometry chain, N x 4 x 4) and factors, a list of (kind, i, j, Z, var) in the order
they are added (kind as posegraph_ref: 0 prior, 1 between, 2 position).  feed() builds the same graph in anything that has add_pose / add_prior /
add_between / add_position: the device wrapper or the NumPy restatement."""
import math

import numpy as np

import posegraph_ref as pr

B = pr.SEGMENT
MAX_SEPARATORS = 256
SIZES = (1, 2, 3, B - 1, B, B + 1, 2 * B, 2 * B + 1, 4 * B + 3)
LAYOUTS = ("none", "one", "separators", "neighbours", "shared", "full")
PRIOR_VAR = (1e-9, 1e-9, 1e-9, 1e-4, 1e-4, 1e-4)      # globalMappingIkdTree.cpp:154
ODOM_VAR = (0.05,) * 6
LOOP_VAR = (0.011, 0.012, 0.013, 0.021, 0.022, 0.023)
POS_VAR = (0.1, 0.2, 0.3)


def pose(w, t):
    T = np.eye(4); T[:3, :3] = pr.so3_exp(np.asarray(w, np.float64)); T[:3, 3] = t
    return T


def truth(N):
    out = []
    for k in range(N):
        phi = 2.0 * math.pi * k / max(N - 1, 8)
        Rz = pr.so3_exp(np.array([0.0, 0.0, phi + 0.5 * math.pi]))
        Rw = pr.so3_exp(np.array([0.05 * math.sin(2 * phi), 0.04 * math.cos(3 * phi), 0.0]))
        T = np.eye(4); T[:3, :3] = Rz @ Rw; T[:3, 3] = [20.0 * math.cos(phi), 20.0 * math.sin(phi), 0.5 * math.sin(3 * phi)]
        out.append(T)
    return out


def loops(N, layout):
    """The loop edges (i, j), i > j as the reference adds them, of a layout at N poses; [] where the layout needs more poses."""
    if layout == "one" and N >= 3:
        return [(N - 1, 0)]
    if layout == "separators" and N >= 2 * B:
        return [(2 * B - 1, B - 1)]
    if layout == "neighbours" and N >= B + 1:
        return [(B, B - 2)]
    if layout == "shared" and N >= 5:
        return [(N - 1, 0), (N - 1, N // 2)]
    if layout == "full":                                      # as many as VPGO_MAX_SEPARATORS allows
        seps = {k for k in range(N) if (k + 1) % B == 0}
        out = []
        for k in range(2, N):
            new = {k, k - 2} - seps
            if len(seps) + len(new) <= MAX_SEPARATORS:
                seps |= new; out.append((k, k - 2))
        return out
    return []


def make(N, layout="none", seed=0, positions=False, loop_list=None):
    rng = np.random.default_rng(1000 * N + 17 * LAYOUTS.index(layout) + seed)
    tr = truth(N)
    noisy = lambda T, sr, st: T @ pose(sr * rng.standard_normal(3), st * rng.standard_normal(3))
    factors = [(pr.PRIOR, 0, 0, noisy(tr[0], 1e-5, 1e-3), np.array(PRIOR_VAR))]      # a prior that disagrees with the first pose (by a third of its sigma): no fixture starts at zero cost
    init = [tr[0].copy()]
    for k in range(1, N):
        Z = noisy(pr.inverse(tr[k - 1]) @ tr[k], 0.002, 0.02)
        factors.append((pr.BETWEEN, k - 1, k, Z, np.array(ODOM_VAR)))
        init.append(init[-1] @ Z)
        if positions and k % 10 == 0:
            factors.append((pr.POSITION, k, k, tr[k][:3, 3] + 0.05 * rng.standard_normal(3), np.array(POS_VAR)))
    for i, j in (loops(N, layout) if loop_list is None else loop_list):
        factors.append((pr.BETWEEN, i, j, noisy(pr.inverse(tr[i]) @ tr[j], 0.001, 0.01), np.array(LOOP_VAR)))
    return {"truth": np.array(tr), "init": np.array(init), "factors": factors, "N": N}


def events(fx):
    """The fixture as the reference builds it, one scan at a time: ("pose", T) then the factors whose keys exist by then."""
    out, done = [], 0
    fac = fx["factors"]
    for k in range(fx["N"]):
        out.append(("pose", fx["init"][k]))
        while done < len(fac) and max(fac[done][1], fac[done][2]) <= k:
            out.append(("factor", fac[done])); done += 1
    assert done == len(fac)
    return out


def add_factor(g, f):
    kind, i, j, Z, var = f
    if kind == pr.PRIOR:
        g.add_prior(i, Z, var)
    elif kind == pr.BETWEEN:
        g.add_between(i, j, Z, var)
    else:
        g.add_position(i, Z, var)


def feed(g, fx, batch=True):
    """batch: all poses, then all factors.  Otherwise in the order of events().  The factor order is the same either way, unless a loop
    factor sits before an odometry factor of a later key -- make() appends loops last, so events() reorders them and so does this."""
    if batch:
        for T in fx["init"]:
            g.add_pose(T)
        for kind, f in [e for e in events(fx) if e[0] == "factor"]:
            add_factor(g, f)
    else:
        for kind, v in events(fx):
            if kind == "pose":
                g.add_pose(v)
            else:
                add_factor(g, v)
    return g


def ordered_factors(fx):
    return [f for kind, f in events(fx) if kind == "factor"]


def content_key(fx):
    """A fixture's identity is its content: the initial values and every factor's numbers."""
    import hashlib
    h = hashlib.sha256(np.ascontiguousarray(fx["init"], np.float64).tobytes())
    for kind, i, j, Z, var in fx["factors"]:
        h.update(np.array([kind, i, j], np.int64).tobytes()); h.update(np.ascontiguousarray(Z, np.float64).tobytes()); h.update(np.ascontiguousarray(var, np.float64).tobytes())
    return h.hexdigest()


def scipy_problem(fx):
    """(residual function, dense Jacobian function, x0, the restatement's graph, the base poses) for scipy.optimize.least_squares"""
    import scipy.sparse as sp
    g = pr.Graph()
    g.poses = [T.copy() for T in fx["init"]]
    g.factors = ordered_factors(fx)
    base = [T.copy() for T in g.poses]
    N = len(base)

    def chart(x):
        blocks = []
        for k in range(N):
            w = x[6 * k:6 * k + 3]
            D = np.zeros((6, 6))
            D[:3, :3] = np.linalg.inv(pr.so3_jri(w, float(np.linalg.norm(w))))
            D[3:, 3:] = pr.so3_exp(w).T
            blocks.append(D)
        return sp.block_diag(blocks, format="csr")

    fun = lambda x: g.linearize(g.moved(x, base), jac=False)[0].ravel()

    def jac(x):
        _, Ji, Jj = g.linearize(g.moved(x, base))
        return (g.jacobian(Ji, Jj) @ chart(x)).tocsr()

    return fun, (lambda x: jac(x).toarray()), np.zeros(6 * N), g, base


def scipy_status(fx):
    """least_squares (`trf`, exact trust-region solver, scipy's default tolerances) on a fixture that needs no bound from it: its status"""
    import scipy.optimize as so
    fun, dense, x0, _, _ = scipy_problem(fx)
    return so.least_squares(fun, x0, jac=dense, method="trf", tr_solver="exact", x_scale=1.0, max_nfev=100).status


_REFERENCE = {}


def scipy_reference(fx):
    """scipy.optimize.least_squares on the restatement's residual from the fixture's initial values, methods `trf` (exact trust-region solver) and `lm`.
    The Jacobian is exact: the restatement's J is taken in the chart at the moved pose, and a step dx of the parameters x (the chart at the
    initial pose) moves that chart by blockdiag(Jr(x_w), Exp(x_w)^T) dx, Jr the inverse of the header's Jri.
    Returns {"poses": trf's solution, "grad": |J^T r|_inf there, "spread": the largest chart-local component between the two solutions,
    "status": (trf, lm)}; cached per fixture."""
    key = content_key(fx)
    if key in _REFERENCE:
        return _REFERENCE[key]
    import scipy.optimize as so
    fun, dense, x0, g, base = scipy_problem(fx)

    tight = dict(xtol=1e-15, ftol=1e-15, gtol=1e-15)
    trf = so.least_squares(fun, x0, jac=dense, method="trf", tr_solver="exact", x_scale=1.0, max_nfev=100, **tight)      # (lsmr stalls on the prior's 1e9 next to the edges' 20)
    lm = so.least_squares(fun, x0, jac=dense, method="lm", x_scale=1.0, max_nfev=100, **tight)
    P_trf, P_lm = g.moved(trf.x, base), g.moved(lm.x, base)
    r, Ji, Jj = g.linearize(P_trf)
    out = {"poses": P_trf, "grad": float(np.abs(g.gradient(r, Ji, Jj)).max()), "status": (trf.status, lm.status),
           "spread": float(max(np.abs(pr.local(a, b)).max() for a, b in zip(P_trf, P_lm))), "cost": float(trf.cost)}
    _REFERENCE[key] = out
    return out
