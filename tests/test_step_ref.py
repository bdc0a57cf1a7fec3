"""The one-step reference (tests/step_ref.py) and the inputs of test_gpu_step.py proved on the CPU, with the oracle as the library under test.

Every window and radius the GPU test uses: the step is accepted (a rejected step leaves the state where it was and proves nothing), the radius selects the
intended branch of the dogleg, the longdouble reference's own backward error is <= 1e-17 (two orders under anything it judges), and the oracle -- a float64
Cholesky with substitutions -- stays inside the bounds the GPU's substituting structures are held to.  A bound the reference alone did not leave room for
would fail here, not on the GPU.
"""
import numpy as np
import pytest

import step_ref as sr

FULL = tuple("K%d" % k for k in sr.KS_FULL)
CASES = [(n, b) for n in sr.WINDOWS for b in ((sr.GN, sr.INTERPOLATED, sr.CAUCHY) if n in FULL else (sr.GN,))]


@pytest.fixture(scope="module")
def refs(oracle):
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = sr.StepRef(oracle, sr.make_window(name, oracle), sr.abi.default_options())
        return cache[name]
    return get


@pytest.mark.parametrize("name,branch", CASES)
def test_oracle_step_meets_the_bounds(oracle, refs, name, branch):
    ref = refs(name)
    assert ref.omega_ref <= 1e-17, ref.omega_ref
    step, radius = sr.one_step(oracle, ref, branch)
    sr.check_step(ref, step, ref.state, branch, radius, False, "oracle %s" % name)


@pytest.mark.parametrize("name", ["K10", "K20", "c2"])
def test_oracle_second_step_meets_the_bounds(oracle, refs, name):
    """Iteration 2: Jacobi scales of the initial state, H, g, d of the state after step 1, the radius of radius_trace."""
    ref2, step, branch, radius = sr.second_step(oracle, oracle, refs(name))
    assert ref2.omega_ref <= 1e-17, ref2.omega_ref
    sr.check_step(ref2, step, ref2.state, branch, radius, False, "oracle %s iteration 2" % name)


def test_read_step_inverts_the_update():
    """read_step against the update rule itself: p + dp, q <- normalize(q (x) (theta / 2, 1)), within read_noise (steps below the state components'
    own size, as a trust-region step's are: the rounding of the stored sum is then that of the state component)."""
    w = sr.synth.make_config(1, L=60)
    rng = np.random.default_rng(3)
    before = w.state_copy()
    K, D = w.K, w.D
    mag = sr.read_noise(w, before, np.ones(D + w.L)) * 2.0 ** 52          # |state component| of the differences
    step = mag * rng.uniform(-0.3, 0.3, D + w.L)
    rot = np.concatenate([np.arange(6 * k + 3, 6 * k + 6) for k in range(K + 1)])
    step[rot] = rng.normal(0, 0.02, len(rot))
    after = {k: v.copy() for k, v in before.items()}
    plus = lambda q, th: (lambda p: p / np.linalg.norm(p))(sr.synth.qmul(q, np.append(0.5 * th, 1.0)))
    for k in range(K):
        after["pose"][k, :3] += step[6 * k: 6 * k + 3]
        after["pose"][k, 3:] = plus(before["pose"][k, 3:], step[6 * k + 3: 6 * k + 6])
        after["speedbias"][k] += step[6 * K + 7 + 9 * k: 6 * K + 16 + 9 * k]
    after["ex_pose"][:3] += step[6 * K: 6 * K + 3]
    after["ex_pose"][3:] = plus(before["ex_pose"][3:], step[6 * K + 3: 6 * K + 6])
    after["td"][0] += step[6 * K + 6]
    after["inv_depth"] += step[D:]
    got = sr.read_step(w, before, after)
    assert np.abs(got).min() > 0 and np.all(np.abs(got - step) <= sr.read_noise(w, before, np.ones(D + w.L)))


def test_omega_and_refinement_on_a_known_system():
    """omega is zero on an exactly representable solution, scales with a perturbation of it, and the refined solve reaches longdouble level on a system of
    the condition the windows have (3e8)."""
    rng = np.random.default_rng(1)
    Q, _ = np.linalg.qr(rng.normal(size=(40, 40)))
    M = (Q * np.logspace(0, 8.5, 40)) @ Q.T
    M = 0.5 * (M + M.T)
    x = np.round(rng.normal(size=40) * 64) / 64
    Ml = M.astype(sr.LD)
    rhs = Ml @ x.astype(sr.LD)
    assert sr.omega(Ml, rhs, x) == 0.0
    x2 = x.copy(); x2[7] *= 1 + 1e-9
    assert 1e-12 < sr.omega(Ml, rhs, x2) < 1e-9
    xr, om = sr.refined_solve(Ml, rhs)
    assert om <= 1e-17 and np.abs(xr - x).max() <= 1e-9 * np.abs(x).max()
