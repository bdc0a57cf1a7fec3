"""ONE trust-region step of the HIP library against an extended-precision solve of the same linear system (tests/step_ref.py).

The trajectory tests see the step's linear algebra -- chain elimination from both ends, W W^T contraction, dense factorisation, chain and landmark back
substitution, dogleg combination -- only through a converged solve (cost to 1e-8, positions to 1e-6 m), and a trust-region loop converges to the same minimum
with an inexact step.  Here max_iterations = 1: the state difference IS the step, and the reference is built from vil_eval_factors alone (pinned factor by
factor in test_gpu_parity.py), so nothing of the oracle judges (it only builds the prior, as everywhere in the suite).

Bounds (step_ref.check_step), omega = componentwise backward error of x = -step / s in M x = rhs over ALL rows, landmarks included:
  * Gauss-Newton branch, structures that SUBSTITUTE through the chain's pivot blocks (three launches per iteration: modes 1, 2, the forced multi-GPU split,
    the dense path): omega <= 20 omega64, omega64 = the float64 numpy route on the same window, 20 = the margin test_gpu_marg.py grants another elimination
    order of one SPD matrix.
  * Gauss-Newton branch, structures whose chain workgroup runs beside the gather or inside a one-launch kernel (0, 1 or 2 launches per iteration): the pose
    rows of the elimination are PRODUCTS with published inverses of the 9 x 9 pivot blocks (vil_prechain.hpp: `fw`, K <= 20), "less accurate by the block's
    condition number" (DESIGN.md 5.1): omega <= 20 omega64 kappa_b, kappa_b computed in numpy from M.
  * Cauchy / interpolated branch: every scaled component within 20 x the float64 route's largest error + the rounding of reading that component back.

A window the upload classifies as "not a chain" (choose_structure: an IMU factor that joins frames more than one apart) is synth's K = 5 window with one
factor's second frame moved from 2 to 3 (step_ref.make_window("dense")) -- no new product code: the dense path over all D columns runs.
"""
import ctypes as C

import numpy as np
import pytest

import step_ref as sr
from mvil_fusion_amd import lib

pytestmark = pytest.mark.gpu

# structure -> (vil_debug_set_launch_mode, vil_debug_set_split, launches per iteration vil_debug_get_launch_structure must report)
STRUCTS = {"default": (0, 0, (0, 1)), "mode1": (1, 0, (3,)), "mode2": (2, 0, (3,)), "mode3": (3, 0, (2,)), "mode4": (4, 0, (1,)), "split": (0, 1, (3,))}
FULL = tuple("K%d" % k for k in sr.KS_FULL)
GN_CASES = [(n, "default") for n in sr.WINDOWS] + [(n, s) for s in STRUCTS if s != "default" for n in FULL]
BRANCH_CASES = [(n, s, b) for n in FULL for s in ("default", "mode2") for b in (sr.INTERPOLATED, sr.CAUCHY)]


@pytest.fixture(scope="module")
def backends(hip):
    made = {"default": hip}
    for name, (mode, split, _) in STRUCTS.items():
        if name != "default":
            be = made[name] = lib.open_vilsolve()
            assert be.lib.vil_debug_set_launch_mode(be.ctx, mode) == 0 and be.lib.vil_debug_set_split(be.ctx, split) == 0
    yield made
    for name, be in made.items():
        if name != "default":
            be.close()


@pytest.fixture(scope="module")
def refs(hip, oracle):
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = sr.StepRef(hip, sr.make_window(name, oracle), sr.abi.default_options())
        return cache[name]
    return get


def ran(be, struct, name):
    """the structure the last solve of `be` launched: (launches per iteration, the chain rows were products with published inverses)"""
    lpi, one = C.c_int32(-1), C.c_int32(-1)
    assert be.lib.vil_debug_get_launch_structure(be.ctx, C.byref(lpi), C.byref(one)) == 0
    want = (3,) if name == "dense" else STRUCTS[struct][2]
    assert lpi.value in want and one.value == (1 if lpi.value < 2 else 0), (struct, name, lpi.value, one.value)
    if struct == "default" and name == "c2":
        assert lpi.value == 0                          # the persistent solve (k_solve): what the flagship window runs
    return lpi.value, lpi.value < 3


@pytest.mark.parametrize("name,struct", GN_CASES)
def test_gauss_newton_step_backward_error(backends, refs, name, struct):
    be, ref = backends[struct], refs(name)
    step, radius = sr.one_step(be, ref, sr.GN)
    lpi, inverse = ran(be, struct, name)
    sr.check_step(ref, step, ref.state, sr.GN, radius, inverse, "%s %s (%d launches)" % (name, struct, lpi))


@pytest.mark.parametrize("name,struct,branch", BRANCH_CASES)
def test_cauchy_and_interpolated_step(backends, refs, name, struct, branch):
    be, ref = backends[struct], refs(name)
    step, radius = sr.one_step(be, ref, branch)
    lpi, inverse = ran(be, struct, name)
    sr.check_step(ref, step, ref.state, branch, radius, inverse, "%s %s (%d launches)" % (name, struct, lpi))


@pytest.mark.parametrize("name,struct", [(n, s) for n in ("K10", "K20") for s in ("default", "mode4")] + [("c2", "default")])
def test_second_step(hip, backends, refs, name, struct):
    """Iteration 2 -- the hand-over between the two system sets, the epoch words inside a resident launch: Jacobi scales of the initial state, H, g, d at the
    state after step 1, mu = min_mu, the radius of radius_trace.  The L = 80 windows have too few sweep roles to take the gather's items as duties, so their
    default structure is the one-launch iteration (k_iter); the persistent solve (k_solve) runs on BASELINE's configs[1] at full size: window "c2"."""
    be = backends[struct]
    ref2, step, branch, radius = sr.second_step(be, hip, refs(name))
    lpi, inverse = ran(be, struct, name)
    sr.check_step(ref2, step, ref2.state, branch, radius, inverse, "%s %s (%d launches) iteration 2" % (name, struct, lpi))


@pytest.mark.parametrize("name,struct", [("K10", s) for s in STRUCTS] + [("c2", "default")])
def test_step_is_bit_reproducible(backends, refs, name, struct):
    be, ref = backends[struct], refs(name)
    a, _ = sr.one_step(be, ref, sr.GN)
    b, _ = sr.one_step(be, ref, sr.GN)
    ran(be, struct, name)
    assert np.array_equal(a, b) and np.abs(a).max() > 0
