"""NumPy restatement of the arithmetic contract of include/vilpgo.h (pose-graph optimisation).  It shares no code with the library.

Every formula takes the scalar functions it needs from a namespace `m` (math for float64, mpmath for the 40-digit checks) and works on
NumPy arrays of either float64 or mpmath numbers, so that the float64 floor of a formula is the difference of two runs of the same code."""
import math

import numpy as np

SMALL_ANGLE = 1e-4
SUM_BLOCK = 256
SEGMENT = 64
LAMBDA_FLOOR = 1e-6
PRIOR, BETWEEN, POSITION = 0, 1, 2


def skew(p):
    z = p[0] * 0
    return np.array([[z, -p[2], p[1]], [p[2], z, -p[0]], [-p[1], p[0], z]], dtype=p.dtype if hasattr(p, "dtype") else None)


def so3_log(A, m=math):
    """(Log(A), theta)"""
    v = np.array([A[2, 1] - A[1, 2], A[0, 2] - A[2, 0], A[1, 0] - A[0, 1]], dtype=A.dtype) / 2
    s = m.sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2])
    c = (((A[0, 0] + A[1, 1]) + A[2, 2]) - 1) / 2
    th = m.atan2(s, c)
    t2 = th * th
    k = 1 + t2 / 6 + 7 * t2 * t2 / 360 if th < SMALL_ANGLE else th / s
    return k * v, th


def so3_jri(w, th, m=math):
    """I + [w]x / 2 + e [w]x^2 with [w]x^2 = w w^T - |w|^2 I"""
    t2 = th * th
    e = 1 / (t2 * 0 + 12) + t2 / 720 if th < SMALL_ANGLE else 1 / t2 - (1 + m.cos(th)) / (2 * th * m.sin(th))
    ww = (w[0] * w[0] + w[1] * w[1]) + w[2] * w[2]
    I = np.eye(3, dtype=w.dtype) if w.dtype != object else np.array([[w[0] * 0 + (1 if r == c else 0) for c in range(3)] for r in range(3)], dtype=object)
    return I + skew(w) / 2 + e * (np.outer(w, w) - ww * I)


def so3_exp(w, m=math):
    t2 = (w[0] * w[0] + w[1] * w[1]) + w[2] * w[2]
    th = m.sqrt(t2)
    if th < SMALL_ANGLE:
        a, b = 1 - t2 / 6, 1 / (t2 * 0 + 2) - t2 / 24
    else:
        sh = m.sin(th / 2)
        a, b = m.sin(th) / th, 2 * sh * sh / t2
    I = np.eye(3, dtype=w.dtype) if w.dtype != object else np.array([[w[0] * 0 + (1 if r == c else 0) for c in range(3)] for r in range(3)], dtype=object)
    return I + a * skew(w) + b * (np.outer(w, w) - t2 * I)


def factor_eval(kind, Ti, Tj, Z, var, m=math, jac=True):
    """Whitened residual (6; a position factor fills three) and the 6 x 6 Jacobians with respect to the first and the second pose."""
    dt = Ti.dtype
    zero = Ti[0, 0] * 0
    r = np.array([zero] * 6, dtype=dt); Ji = np.array([[zero] * 6] * 6, dtype=dt); Jj = np.array([[zero] * 6] * 6, dtype=dt)
    sig = np.array([m.sqrt(v) for v in var], dtype=dt)
    Ri, ti = Ti[:3, :3], Ti[:3, 3]
    if kind == POSITION:
        r[:3] = (ti - Z) / sig
        Ji[:3, 3:] = Ri / sig[:, None]
        return r, Ji, Jj
    Zr, Zt = Z[:3, :3], Z[:3, 3]
    if kind == PRIOR:
        A = Zr.T @ Ri
        w, th = so3_log(A, m)
        r[:3] = w / sig[:3]; r[3:] = (Zr.T @ (ti - Zt)) / sig[3:]
        if jac:
            Ji[:3, :3] = so3_jri(w, th, m) / sig[:3, None]; Ji[3:, 3:] = A / sig[3:, None]
        return r, Ji, Jj
    Rj, tj = Tj[:3, :3], Tj[:3, 3]
    Rij = Ri.T @ Rj
    A = Zr.T @ Rij
    p = Ri.T @ (tj - ti)
    w, th = so3_log(A, m)
    r[:3] = w / sig[:3]; r[3:] = (Zr.T @ (p - Zt)) / sig[3:]
    if jac:
        Jr = so3_jri(w, th, m)
        Jj[:3, :3] = Jr / sig[:3, None]; Jj[3:, 3:] = A / sig[3:, None]
        Ji[:3, :3] = -(Jr @ Rij.T) / sig[:3, None]; Ji[3:, :3] = (Zr.T @ skew(p)) / sig[3:, None]; Ji[3:, 3:] = -Zr.T / sig[3:, None]
    return r, Ji, Jj


def retract(T, d, m=math):
    """t <- t + R dv, R <- R Exp(dw), R <- R (3 I - R^T R) / 2"""
    out = T.copy()
    R = T[:3, :3]
    out[:3, 3] = T[:3, 3] + R @ d[3:]
    M = R @ so3_exp(d[:3], m)
    out[:3, :3] = (M @ (3 * np.eye(3) - M.T @ M)) / 2
    return out


def local(Ta, Tb, m=math):
    """The step d with retract(Ta, d) = Tb (up to the re-orthonormalisation)."""
    w, _ = so3_log(Ta[:3, :3].T @ Tb[:3, :3], m)
    return np.concatenate([w, Ta[:3, :3].T @ (Tb[:3, 3] - Ta[:3, 3])])


def inverse(T):
    out = np.eye(4); out[:3, :3] = T[:3, :3].T; out[:3, 3] = -T[:3, :3].T @ T[:3, 3]
    return out


class Graph:
    """poses: list of 4 x 4; factors: list of (kind, i, j, Z, var), Z 4 x 4 or, for a position factor, 3 long."""

    def __init__(self):
        self.poses, self.factors = [], []

    def add_pose(self, T):
        self.poses.append(np.array(T, np.float64)); return len(self.poses) - 1

    def add_prior(self, i, Z, var):
        self.factors.append((PRIOR, i, i, np.array(Z, np.float64), np.array(var, np.float64)))

    def add_between(self, i, j, Z, var):
        self.factors.append((BETWEEN, i, j, np.array(Z, np.float64), np.array(var, np.float64)))

    def add_position(self, i, z, var):
        self.factors.append((POSITION, i, i, np.array(z, np.float64), np.array(var, np.float64)))

    def linearize(self, poses=None, jac=True):
        """(r F x 6, J_i F x 6 x 6, J_j F x 6 x 6)"""
        P = self.poses if poses is None else poses
        F = len(self.factors)
        r = np.zeros((F, 6)); Ji = np.zeros((F, 6, 6)); Jj = np.zeros((F, 6, 6))
        for f, (kind, i, j, Z, var) in enumerate(self.factors):
            r[f], Ji[f], Jj[f] = factor_eval(kind, P[i], P[j], Z, var, jac=jac)
        return r, Ji, Jj

    @staticmethod
    def cost_of(r):
        """1/2 sum |r|^2: a factor's term is the sequential sum of its six squares, blocks of 256 factors, then the partials, all from 0.0"""
        terms = []
        for row in r:
            c = 0.0
            for v in row:
                c = c + v * v
            terms.append(0.5 * c)
        total = 0.0
        for b0 in range(0, len(terms), SUM_BLOCK):
            acc = 0.0
            for v in terms[b0:b0 + SUM_BLOCK]:
                acc = acc + v
            total = total + acc
        return total

    def gradient(self, r, Ji, Jj):
        """N x 6: per pose the sum of J^T r over its factors in ascending factor index"""
        g = np.zeros((len(self.poses), 6))
        for f, (kind, i, j, _, _) in enumerate(self.factors):
            g[i] = g[i] + Ji[f].T @ r[f]
            if kind == BETWEEN:
                g[j] = g[j] + Jj[f].T @ r[f]
        return g

    def jacobian(self, Ji, Jj):
        """scipy.sparse CSR, 6 F x 6 N"""
        import scipy.sparse as sp
        rows, cols, vals = [], [], []
        rr, cc = np.meshgrid(np.arange(6), np.arange(6), indexing="ij")
        for f, (kind, i, j, _, _) in enumerate(self.factors):
            rows.append((6 * f + rr).ravel()); cols.append((6 * i + cc).ravel()); vals.append(Ji[f].ravel())
            if kind == BETWEEN:
                rows.append((6 * f + rr).ravel()); cols.append((6 * j + cc).ravel()); vals.append(Jj[f].ravel())
        return sp.csr_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))), shape=(6 * len(self.factors), 6 * len(self.poses)))

    def moved(self, x, base=None):
        """The poses after the step x (6 N) from base."""
        base = self.poses if base is None else base
        return [retract(T, x[6 * k:6 * k + 6]) for k, T in enumerate(base)]

    def residual_fn(self, base=None):
        """x -> stacked whitened residuals at retract(base, x), and its Jacobian at x = 0 only is J; for scipy the Jacobian is taken at the
        moved poses and is exact for the chart centred there, which differs from d/dx by second-order terms in x: scipy gets '2-point'."""
        base = [T.copy() for T in (self.poses if base is None else base)]
        return lambda x: self.linearize(self.moved(x, base), jac=False)[0].ravel()

    def optimize(self, max_iterations=20, initial_lambda=1e-5, step_tolerance=1e-10, cost_tolerance=1e-12):
        """The minimiser of the header with a sparse direct solve.  Returns (iterations, initial cost, final cost, termination)."""
        import scipy.sparse as sp
        import scipy.sparse.linalg as spl
        lam, nu = initial_lambda, 2.0
        r, Ji, Jj = self.linearize()
        cost = cost0 = self.cost_of(r)
        it, term = 0, 3
        while it < max_iterations:
            it += 1
            J = self.jacobian(Ji, Jj)
            g = J.T @ r.ravel()
            H = (J.T @ J + lam * sp.identity(J.shape[1])).tocsc()
            try:
                d = spl.splu(H).solve(-g)
            except RuntimeError:
                d = None
            ok = d is not None and np.all(np.isfinite(d))
            if ok:
                cand = self.moved(d)
                r2, Ji2, Jj2 = self.linearize(cand)
                c2 = self.cost_of(r2)
                pred = 0.5 * float(d @ (lam * d - g))
                maxd = float(np.abs(d).max())
                ok = np.isfinite(c2) and pred > 0 and (cost - c2) / pred > 0
            if ok:
                rho, rel = (cost - c2) / pred, (cost - c2) / cost
                self.poses, r, Ji, Jj, cost = cand, r2, Ji2, Jj2, c2
                lam, nu = lam * max(1.0 / 3.0, 1.0 - (2.0 * rho - 1.0) ** 3), 2.0
                if maxd < step_tolerance:
                    term = 1; break
                if rel < cost_tolerance:
                    term = 2; break
            else:
                lam, nu = max(lam * nu, LAMBDA_FLOOR), 2.0 * nu
                if d is not None and np.all(np.isfinite(d)) and maxd < step_tolerance:
                    term = 1; break
        return it, cost0, cost, term
