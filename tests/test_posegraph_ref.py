"""The NumPy restatement of include/vilpgo.h (tests/posegraph_ref.py) earns its place before the device is compared with it: its analytic Jacobians
against central differences of its own residual in 40-digit mpmath, and scipy.optimize.least_squares on its residual for every fixture the GPU
tests use (status > 0), with its figures recorded for the fixtures the GPU tests converge on.  The figures scipy reaches are the GPU tests' bounds (posegraph_fixtures.scipy_reference); recorded here with this seed set:
  N 129 shared      |J^T r|_inf 1.2e-09   lm / trf spread 9.6e-09
  N 129 one         |J^T r|_inf 4.4e-10   lm / trf spread 6.8e-10
  N  65 neighbours  |J^T r|_inf 1.9e-09   lm / trf spread 6.6e-09
(the prior's rows are 3e4 large, 1 / sqrt(1e-9): the gradient's rounding floor sits near 1e-9, not near 1e-13)"""
import mpmath
import numpy as np
import pytest

import posegraph_fixtures as pf
import posegraph_ref as pr

T_ = pr.SMALL_ANGLE
ANGLES = [0.0, T_ * (1 - 1e-3), T_, T_ * (1 + 1e-3), 3.0]
B = pr.SEGMENT


def to_mp(a):
    return np.array([mpmath.mpf(float(v)) for v in np.asarray(a, np.float64).ravel()], dtype=object).reshape(np.shape(a))


def mp_pose(w, t):
    T = to_mp(np.eye(4)); T[:3, :3] = pr.so3_exp(to_mp(w), mpmath); T[:3, 3] = to_mp(t)
    return T


def mp_inverse(T):
    out = to_mp(np.eye(4)); out[:3, :3] = T[:3, :3].T; out[:3, 3] = -(T[:3, :3].T @ T[:3, 3])
    return out


def case(kind, angle, seed):
    """Two poses and a measurement whose residual rotation has the given angle, with variances that all differ -- in 40 digits, so that the
    rotations are orthonormal to 1e-40: the formulas are derivatives on SO(3), and a matrix that is orthonormal to 1e-16 only shifts them by
    that times 1 / angle."""
    rng = np.random.default_rng(seed)
    Ti, Tj = mp_pose(0.7 * rng.standard_normal(3), 5 * rng.standard_normal(3)), mp_pose(0.7 * rng.standard_normal(3), 5 * rng.standard_normal(3))
    u = rng.standard_normal(3); u = to_mp(u) / mpmath.sqrt(sum(mpmath.mpf(float(v)) ** 2 for v in u))
    D = to_mp(np.eye(4)); D[:3, :3] = pr.so3_exp(mpmath.mpf(angle) * u, mpmath); D[:3, 3] = to_mp(0.2 * rng.standard_normal(3))
    var = to_mp(0.01 + rng.random(6))
    if kind == pr.PRIOR:
        return Ti, Ti, Ti @ mp_inverse(D), var
    if kind == pr.BETWEEN:
        return Ti, Tj, mp_inverse(Ti) @ Tj @ mp_inverse(D), var
    return Ti, Ti, Ti[:3, 3] + to_mp(rng.standard_normal(3)), var[:3]


def to_f64(a):
    return np.array([float(v) for v in np.asarray(a, dtype=object).ravel()], np.float64).reshape(np.shape(a))


@pytest.mark.parametrize("angle", ANGLES)
@pytest.mark.parametrize("kind", [pr.PRIOR, pr.BETWEEN, pr.POSITION])
def test_jacobians_against_central_differences_at_40_digits(kind, angle):
    mpmath.mp.dps = 40
    mTi, mTj, mZ, mvar = case(kind, angle, 7 + int(1e6 * angle) % 1000)
    r64, Ji64, Jj64 = pr.factor_eval(kind, to_f64(mTi), to_f64(mTj), to_f64(mZ), to_f64(mvar))
    if kind != pr.POSITION:
        th = pr.so3_log(mZ[:3, :3].T @ (mTi[:3, :3] if kind == pr.PRIOR else mTi[:3, :3].T @ mTj[:3, :3]), mpmath)[1]
        assert abs(th - mpmath.mpf(angle)) <= mpmath.mpf(10) ** -20, (th, angle)      # the case sits where it says (below the threshold Exp's own series builds it: 8e-23)
    _, Jim, Jjm = pr.factor_eval(kind, mTi, mTj, mZ, mvar, m=mpmath)
    h = mpmath.mpf(10) ** -10
    num = [np.zeros((6, 6), dtype=object), np.zeros((6, 6), dtype=object)]
    for side in (0, 1):
        for c in range(6):
            d = to_mp(np.zeros(6)); d[c] = h
            plus, minus = (pr.retract(mTi if side == 0 else mTj, s * d, mpmath) for s in (1, -1))
            if kind == pr.BETWEEN:
                args = lambda T: (T, mTj) if side == 0 else (mTi, T)
            else:
                args = lambda T: (T, T) if side == 0 else (mTi, mTi)       # a unary factor does not see its second argument
            rp = pr.factor_eval(kind, *args(plus), mZ, mvar, m=mpmath, jac=False)[0]
            rm = pr.factor_eval(kind, *args(minus), mZ, mvar, m=mpmath, jac=False)[0]
            num[side][:, c] = (rp - rm) / (2 * h)
    amax = lambda a: float(max(abs(v) for v in np.asarray(a, dtype=object).ravel()))
    scale = max(1.0, amax(Jim), amax(Jjm))
    e_formula = max(amax(Jim - num[0]), amax(Jjm - num[1]))
    e_f64 = max(amax(to_mp(Ji64) - num[0]), amax(to_mp(Jj64) - num[1]))
    print("kind %d angle %.6g: formula against differences %.2e, float64 against differences %.2e (scale %.3g)" % (kind, angle, e_formula, e_f64, scale))
    # differences of step 1e-10 at 40 digits: truncation 1e-20 x third derivative; a step that straddles the threshold adds the series' own
    # truncation (2e-27 x angle) / step.  float64: the inputs' rounding and a few dozen roundings of entries up to `scale`, amplified by
    # 1 / sin^2(3.0) = 50 at 3.0 rad.
    assert e_formula <= 1e-16 * scale and e_f64 <= 1e-12 * scale


def test_cost_sum_order_and_gradient():
    fx = pf.make(4 * B + 3, "full", positions=True)
    g = pf.feed(pr.Graph(), fx)
    r, Ji, Jj = g.linearize()
    assert len(r) > pr.SUM_BLOCK and abs(g.cost_of(r) - 0.5 * float((r * r).sum())) <= 1e-13 * g.cost_of(r)
    J = g.jacobian(Ji, Jj)
    assert np.abs(g.gradient(r, Ji, Jj).ravel() - J.T @ r.ravel()).max() <= 1e-12 * np.abs(J.T @ r.ravel()).max()


@pytest.mark.parametrize("N,layout", [(2 * B + 1, "shared"), (2 * B + 1, "one"), (B + 1, "neighbours")])
def test_scipy_converges_on_the_fixtures_and_records_the_bounds(N, layout):
    fx = pf.make(N, layout, positions=True)
    ref = pf.scipy_reference(fx)
    print("N %d %s: status trf %d lm %d, |J^T r|_inf %.3e, lm / trf spread %.3e, cost %.12g" % (N, layout, ref["status"][0], ref["status"][1], ref["grad"], ref["spread"], ref["cost"]))
    assert ref["status"][0] > 0 and ref["status"][1] > 0
    own = pf.feed(pr.Graph(), fx)
    it, c0, c1, term = own.optimize(cost_tolerance=0.0, step_tolerance=1e-11)
    dist = float(max(np.abs(pr.local(a, b)).max() for a, b in zip(ref["poses"], own.poses)))
    print("    the restatement's own minimiser: %d iterations, termination %d, cost %.12g, distance to scipy %.3e" % (it, term, c1, dist))
    assert term == 1 and it < 20 and abs(c1 - ref["cost"]) <= 1e-12 * c1 and dist <= 10 * ref["spread"]


OTHER_FIXTURES = [(B + 1, "one", 0, True), (12, "none", 3, False), (2 * B + 1, "shared", 0, True), (9, "one", 0, False)]      # error paths, the chain of the verified-loop test, reproducibility / incremental, vpgo_relative


@pytest.mark.parametrize("N,layout,seed,positions", [(N, layout, 0, False) for N in pf.SIZES for layout in pf.LAYOUTS] + OTHER_FIXTURES)
def test_scipy_converges_on_every_other_fixture_of_the_gpu_tests(N, layout, seed, positions):
    """The fixtures no bound is taken from -- the 54 of the one-step test and those of the error-path, reproducibility, incremental, vpgo_relative
    and verified-loop tests (the last without its loop factor, which only a device produces): well posed, scipy stops with a status > 0."""
    status = pf.scipy_status(pf.make(N, layout, seed=seed, positions=positions))
    assert status > 0, (N, layout, status)
