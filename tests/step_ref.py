"""One trust-region step in extended precision (test infrastructure, numpy only).

Everything the library does between the linearisation and the candidate state -- chain elimination, Schur contraction, dense factorisation, the back
substitutions, the dogleg combination -- is ONE linear solve and one blend of two vectors.  This module restates that step over ALL free parameters
(no Schur complement, no elimination order of its own) from the per-factor residuals / Jacobians of a backend's eval_factors (numpy_ref.factor_list),
twice: in np.longdouble (64-bit mantissa, the judge) and in float64 by the same route (the floor any float64 implementation is measured against).

    s        = 1 / (1 + sqrt(diag H))                  Jacobi scaling (ones with jacobi_scaling = 0); fixed at the solve's initial state
    d        = sqrt(clip(s^2 diag H, 1e-6, 1e32))      dogleg diagonal
    M        = diag(s) H diag(s) + mu diag(d^2),  rhs = s g
    gradient = rhs / d,  alpha = |gradient|^2 / (v^T diag(s) H diag(s) v),  v = gradient / d
    gn       = -d M^-1 rhs
    step     = s (cg gradient + cn gn) / d             (cg, cn): Gauss-Newton / Cauchy / interpolated branch of the traditional dogleg

The metric of the Gauss-Newton branch is the componentwise (Oettli-Prager) backward error of x = -step / s in M x = rhs: independent of cond(M) ~ 3e8,
it resolves 1e-15 where a converged trajectory resolves 1e-8.  Shares no code with oracle/ or the kernels.
"""
import numpy as np

import numpy_ref as nr
from mvil_fusion_amd import abi, synth

LD = np.longdouble
SIZE = {"pose": 6, "sb": 9, "ex": 6, "td": 1, "lam": 1}
GN, INTERPOLATED, CAUCHY = "gauss_newton", "interpolated", "cauchy"
MARGIN = 20.0          # what test_gpu_marg.py grants a different elimination order of the same SPD matrix over the float64 floor
KS = (4, 5, 7, 9, 10, 11, 12, 13, 14, 15, 16, 18, 20)          # the path-switch list of test_window_sizes_around_the_path_switches + 10, 20
KS_FULL = (5, 10, 13, 20)                                      # every structure, every branch
WINDOWS = tuple("K%d" % k for k in KS) + ("K7s564", "consts", "c1", "dense", "c2")


def make_window(name, oracle):
    """The windows of the one-step tests, by name (a fresh copy per call: a solve moves the state in place)."""
    pf = lambda pre: oracle.marginalize(pre).to_prior()
    small = dict(L=80, n_plane=600, n_edge=200)
    if name == "c2":                                   # BASELINE's configs[1] at full size: the window whose whole solve is ONE resident launch (k_solve)
        return synth.make_config(2, prior_fn=pf)
    if name == "c1":                                   # prior-less: 4-dof gauge null space held by mu d^2 alone
        return synth.make_config(1, L=60)
    if name == "K7s564":                               # profiles/r06_fuzz.txt's one mismatch, built as tools/fuzz_parity.py builds it
        return synth.make_config(2, prior_fn=pf, K=7, seed_offset=564000, **small)
    if name == "consts":                               # the constancy rules of test_linearize_parity[small_consts]
        w = synth.make_config(2, prior_fn=pf, K=10, **small)
        w.pose_const[w.K - 2] = 1; w.sb_const[w.K - 2] = 1; w.ex_const = 1; w.td_const = 1
        return w
    if name == "dense":                                # an IMU factor that joins frames 1 and 3: "not a chain" to the upload, the dense path over all D columns runs
        w = synth.make_config(2, prior_fn=pf, K=5, **small)
        w.imu_j = w.imu_j.copy(); w.imu_j[1] = 3
        return w
    return synth.make_config(2, prior_fn=pf, K=int(name[1:]), **small)


def free_index(w):
    """key -> first column in the library's layout [pose 6K | ex 6 | td 1 | speed-bias 9K | landmarks L] of every FREE block (landmarks: with an observation)."""
    index = nr.camera_index(w)
    obs = np.bincount(w.vis_l, minlength=w.L) if w.L else np.zeros(0, int)
    for l in range(w.L):
        if not w.lm_const[l] and obs[l] > 0:
            index[("lam", l)] = w.D + l
    return index


def corrected_groups(facs, index):
    """The loss-corrected Jacobian rows and residuals of every factor over its free columns (float64: the corrector runs once, for both routes), as
    (columns, rows, residuals); consecutive factors on the same columns (the LiDAR points of one pose) are stacked into one group."""
    out, held, rows, res = [], None, [], []
    for kind, a, r, blocks in facs:
        _, rc, Jc = nr.corrected(kind, a, np.asarray(r, float), [B for _, B in blocks])
        keep = [(index[k], J) for (k, _), J in zip(blocks, Jc) if k in index]
        if not keep:
            continue
        cols = tuple(q for c, J in keep for q in range(c, c + J.shape[1]))
        assert len(set(cols)) == len(cols)          # (no factor names a block twice)
        if cols != held:
            if held is not None:
                out.append((np.array(held), np.vstack(rows), np.concatenate(res)))
            held, rows, res = cols, [], []
        rows.append(np.hstack([J for _, J in keep])); res.append(np.asarray(rc, float))
    if held is not None:
        out.append((np.array(held), np.vstack(rows), np.concatenate(res)))
    return out


def assemble(groups, N, dtype):
    """H = sum J^T J, g = sum J^T r, the corrected J, r cast to `dtype` before the products."""
    H, g = np.zeros((N, N), dtype), np.zeros(N, dtype)
    for cols, J, r in groups:
        Jf, rf = J.astype(dtype), r.astype(dtype)
        H[np.ix_(cols, cols)] += Jf.T @ Jf
        g[cols] += Jf.T @ rf
    return H, g


def omega(M, rhs, x):
    """Oettli-Prager componentwise backward error max_i |rhs - M x|_i / (|M| |x| + |rhs|)_i, in longdouble."""
    M, rhs, x = np.asarray(M, LD), np.asarray(rhs, LD), np.asarray(x, LD)
    num, den = np.abs(rhs - M @ x), np.abs(M) @ np.abs(x) + np.abs(rhs)
    ok = den > 0
    assert np.all(num[~ok] == 0)
    return float((num[ok] / den[ok]).max())


def refined_solve(M, rhs, rounds=12):
    """M x = rhs: float64 LU, then iterative refinement with residuals formed in longdouble until the backward error no longer falls."""
    M64 = np.asarray(M, np.float64)
    x = np.linalg.solve(M64, np.asarray(rhs, np.float64)).astype(LD)
    best = omega(M, rhs, x)
    for _ in range(rounds):
        y = x + np.linalg.solve(M64, np.asarray(rhs - M @ x, np.float64)).astype(LD)
        om = omega(M, rhs, y)
        if not om < best:
            break
        x, best = y, om
    return x, best


class Route:
    """The first-iteration quantities of the dogleg on one linearisation, in one precision.  s: the Jacobi scales of the solve's initial state (None: form them here)."""

    def __init__(self, H, g, jacobi, mu, dtype, s=None):
        self.dtype = dtype
        dg = np.diag(H).copy()
        one = dtype(1)
        self.s = s if s is not None else (one / (one + np.sqrt(dg)) if jacobi else np.ones(len(dg), dtype))
        self.d = np.sqrt(np.clip(self.s * self.s * dg, dtype(1e-6), dtype(1e32)))
        self.Hs = self.s[:, None] * H * self.s[None, :]
        self.M = self.Hs + dtype(mu) * np.diag(self.d * self.d)
        self.rhs = self.s * g
        self.gradient = self.rhs / self.d
        v = self.gradient / self.d
        self.g_norm = np.sqrt(self.gradient @ self.gradient)
        self.alpha = (self.gradient @ self.gradient) / (v @ self.Hs @ v)
        if dtype is LD:
            self.x, _ = refined_solve(self.M, self.rhs)
        else:
            self.x = np.linalg.solve(self.M, self.rhs)
        self.gn = -self.d * self.x
        self.gn_norm = np.sqrt(self.gn @ self.gn)

    def dogleg(self, radius):
        """(branch, step / s): the traditional dogleg's three branches at `radius` (a float64 value: what the library is handed)."""
        t = self.dtype
        radius = t(radius)
        if self.gn_norm <= radius:
            branch, cg, cn = GN, t(0), t(1)
        elif self.g_norm * self.alpha >= radius:
            branch, cg, cn = CAUCHY, -(radius / self.g_norm), t(0)
        else:
            # the point of the segment a -> b (a = Cauchy point, b = Gauss-Newton step) at distance `radius`: |a + beta (b - a)| = radius, the root in [0, 1]
            # of |b - a|^2 beta^2 + 2 c beta - (radius^2 - |a|^2) = 0, c = a . (b - a), taken in the form without cancellation
            a, b = -self.alpha * self.gradient, self.gn
            e = b - a
            c, e2, gap = a @ e, e @ e, radius * radius - a @ a
            root = np.sqrt(c * c + e2 * gap)
            beta = (root - c) / e2 if c <= 0 else gap / (root + c)
            branch, cg, cn = INTERPOLATED, -self.alpha * (1 - beta), beta
        return branch, (cg * self.gradient + cn * self.gn) / self.d


class StepRef:
    """Both routes on one window at one state.  first: the StepRef of the solve's initial state when this is a later iteration (its Jacobi scales are kept)."""

    def __init__(self, backend, w, opts, first=None):
        self.w, self.N, self.index, self.state = w, w.D + w.L, free_index(w), w.state_copy()
        assert first is None or first.index == self.index
        self.cols = np.array(sorted(c + q for k, c in self.index.items() for q in range(SIZE[k[0]])))
        groups = corrected_groups(nr.factor_list(backend, w, opts), self.index)
        mu = opts.min_mu
        Hl, gl = assemble(groups, self.N, LD)
        H6, g6 = assemble(groups, self.N, np.float64)
        sub = np.ix_(self.cols, self.cols)
        self.ld = Route(Hl[sub], gl[self.cols], opts.jacobi_scaling, mu, LD, None if first is None else first.ld.s)
        self.f64 = Route(H6[sub], g6[self.cols], opts.jacobi_scaling, mu, np.float64, None if first is None else first.f64.s)
        self.omega_ref = omega(self.ld.M, self.ld.rhs, self.ld.x)
        self.omega64 = omega(self.ld.M, self.ld.rhs, self.f64.x)
        self.kappa_b = pivot_block_condition(self)

    def full(self, v):
        out = np.zeros(self.N, np.asarray(v).dtype)
        out[self.cols] = v
        return out

    def radius(self, branch):
        """The initial_radius that makes the library take `branch` (float64)."""
        cauchy = float(self.ld.alpha * self.ld.g_norm)
        return {GN: 1e16, INTERPOLATED: float(np.sqrt(cauchy * float(self.ld.gn_norm))), CAUCHY: 0.5 * cauchy}[branch]


def pivot_block_condition(ref):
    """kappa_b: the largest 2-norm condition number among the 9 x 9 pivot blocks of the two-ended block elimination of the chain (speed-bias) part of M:
    blocks 0 .. K/2 - 1 forwards, K - 1 .. K/2 + 1 backwards, then the middle block.  A constant speed-bias block is an identity block without couplings."""
    K, M = ref.w.K, np.asarray(ref.ld.M, np.float64)
    pos = {c: i for i, c in enumerate(ref.cols)}

    def blk(a, b):
        if ("sb", a) not in ref.index or ("sb", b) not in ref.index:
            return np.eye(9) if a == b else np.zeros((9, 9))
        ia, ib = pos[ref.index[("sb", a)]], pos[ref.index[("sb", b)]]
        return M[ia: ia + 9, ib: ib + 9]
    m, piv = K >> 1, {}
    for k in range(m):
        piv[k] = blk(k, k) - (blk(k, k - 1) @ np.linalg.solve(piv[k - 1], blk(k - 1, k)) if k else 0.0)
    for k in range(K - 1, m, -1):
        piv[k] = blk(k, k) - (blk(k, k + 1) @ np.linalg.solve(piv[k + 1], blk(k + 1, k)) if k < K - 1 else 0.0)
    piv[m] = blk(m, m)
    if m - 1 >= 0:
        piv[m] = piv[m] - blk(m, m - 1) @ np.linalg.solve(piv[m - 1], blk(m - 1, m))
    if m + 1 <= K - 1:
        piv[m] = piv[m] - blk(m, m + 1) @ np.linalg.solve(piv[m + 1], blk(m + 1, m))
    assert len(piv) == K
    return float(max(np.linalg.cond(p) for p in piv.values()))


def _tangent(q0, q1):
    """theta of q1 = normalize(q0 (x) (theta / 2, 1)), quaternions [x y z w]: 2 vec(q0^-1 (x) q1) / w."""
    dq = synth.qmul(np.array([-q0[0], -q0[1], -q0[2], q0[3]]), q1)
    return 2.0 * dq[:3] / dq[3]


def read_step(w, before, after):
    """The tangent step the library applied between two state_copy() images, in the layout of free_index."""
    K, D = w.K, w.D
    out = np.zeros(D + w.L)
    for k in range(K):
        out[6 * k: 6 * k + 3] = after["pose"][k, :3] - before["pose"][k, :3]
        out[6 * k + 3: 6 * k + 6] = _tangent(before["pose"][k, 3:], after["pose"][k, 3:])
        out[6 * K + 7 + 9 * k: 6 * K + 16 + 9 * k] = after["speedbias"][k] - before["speedbias"][k]
    out[6 * K: 6 * K + 3] = after["ex_pose"][:3] - before["ex_pose"][:3]
    out[6 * K + 3: 6 * K + 6] = _tangent(before["ex_pose"][3:], after["ex_pose"][3:])
    out[6 * K + 6] = after["td"][0] - before["td"][0]
    out[D:] = after["inv_depth"] - before["inv_depth"]
    return out


def read_noise(w, before, scaling):
    """Rounding of read_step per SCALED component (step / s): the state is stored in float64, so a difference carries 2^-52 |state component| and a rotation
    read back through a unit quaternion 2^-50.  scaling: s in the layout of free_index."""
    K, D = w.K, w.D
    mag = np.zeros(D + w.L)
    for k in range(K):
        mag[6 * k: 6 * k + 3] = 2.0 ** -52 * np.abs(before["pose"][k, :3])
        mag[6 * k + 3: 6 * k + 6] = 2.0 ** -50
        mag[6 * K + 7 + 9 * k: 6 * K + 16 + 9 * k] = 2.0 ** -52 * np.abs(before["speedbias"][k])
    mag[6 * K: 6 * K + 3] = 2.0 ** -52 * np.abs(before["ex_pose"][:3])
    mag[6 * K + 3: 6 * K + 6] = 2.0 ** -50
    mag[6 * K + 6] = 2.0 ** -52 * abs(before["td"][0])
    mag[D:] = 2.0 ** -52 * np.abs(before["inv_depth"])
    return mag / np.asarray(scaling, np.float64)


def check_step(ref, step, before, branch, radius, inverse_products, tag):
    """The assertions of one case.  ref: StepRef at the state the step was taken from; step: read_step of what the library applied; radius: what it was handed.
    inverse_products: the structure multiplies the chain rows by published inverses of the pivot blocks -- its backward error may exceed the
    floor by their condition number kappa_b; every other structure substitutes and is held to the floor itself.  Returns (omega or None, forward error)."""
    free = np.zeros(ref.N, bool); free[ref.cols] = True
    assert np.all(step[~free] == 0.0), "a constant parameter moved"
    s = np.asarray(ref.ld.s, np.float64)
    br_ld, y_ld = ref.ld.dogleg(radius)
    br_64, y_64 = ref.f64.dogleg(radius)
    assert br_ld == branch and br_64 == branch, (br_ld, br_64, branch)
    y = step[ref.cols] / s                                           # scaled components of the library's step
    err = np.abs(y.astype(LD) - y_ld)
    err64 = float(np.abs(y_64.astype(LD) - y_ld).max())
    fwd = float(err.max() / np.abs(y_ld).max())
    om = None
    if branch == GN:
        om = omega(ref.ld.M, ref.ld.rhs, -y)
        bound = MARGIN * ref.omega64 * (ref.kappa_b if inverse_products else 1.0)
    print("%s %s: omega %s omega64 %.3e ratio %s kappa_b %.3e forward error %.3e (float64 route %.3e) of max|step / s|" % (
        tag, branch, "%.3e" % om if om is not None else "-", ref.omega64, "%.2f" % (om / ref.omega64) if om is not None else "-", ref.kappa_b,
        fwd, err64 / float(np.abs(y_ld).max())))
    if branch == GN:
        assert om <= bound, (tag, om, ref.omega64, ref.kappa_b, bound)
    else:
        noise = read_noise(ref.w, before, ref.full(s) + ~free)[ref.cols]
        over = err - (MARGIN * err64 + noise)
        assert np.all(over <= 0), (tag, branch, float(err.max()), err64, float(noise.max()))
    return om, fwd


def one_step(backend, ref, branch):
    """One iteration of `backend` from ref's state at the radius that selects `branch`; the window is left at ref's state.  Returns (step, radius)."""
    w = ref.w
    w.set_state(ref.state)
    radius = ref.radius(branch)
    summ = backend.solve(w, abi.default_options(max_iterations=1, initial_radius=radius))
    after = w.state_copy()
    w.set_state(ref.state)
    assert (summ.iterations, summ.successful_steps) == (1, 1), (summ.iterations, summ.successful_steps)      # otherwise the state never moved
    return read_step(w, ref.state, after), radius


def second_step(backend, ref_backend, ref):
    """Iteration 2 of a solve from ref's state: one solve capped at one iteration gives the state it starts from (the libraries are bit-reproducible), one capped
    at two the state it ends in.  Returns (StepRef at the state after step 1 with the initial state's Jacobi scales, step, branch, radius of iteration 2)."""
    w = ref.w
    w.set_state(ref.state)
    s1 = backend.solve(w, abi.default_options(max_iterations=1))
    mid = w.state_copy()
    w.set_state(ref.state)
    s2 = backend.solve(w, abi.default_options(max_iterations=2))
    end = w.state_copy()
    assert s1.successful_steps == 1 and (s2.iterations, s2.successful_steps) == (2, 2), (s1.successful_steps, s2.iterations, s2.successful_steps)
    w.set_state(mid)
    ref2 = StepRef(ref_backend, w, abi.default_options(), first=ref)
    w.set_state(ref.state)
    radius = float(s2.radius_trace[1])
    return ref2, read_step(w, mid, end), ref2.ld.dogleg(radius)[0], radius
