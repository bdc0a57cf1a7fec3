"""The chain's W W^T leaves the pose system on the dense factorisation's REGISTER tiles (vil_step.hpp: ww_tiles_load / ww_tiles_sub as the factorisation's PRE
functor; vil_prechain.hpp: ww_idx, the lane-major tile layout the tile workgroups write).

1. The subtraction plus the factorisation by themselves (vil_debug_dense_solve_ww): A = M' + S WW S goes in, WW through the shipping index function, and the factor
   and the solution of M' must come out -- to the bounds test_gpu_dense_solve.py holds the factorisation alone to (backward error <= 1e-13 |M'|, residual
   <= 1e-12 |M'| |x|: the subtraction adds one rounding of an entry of size 2 |M'|, 4e-16 |M'|).  |S WW S| ~ |M'|, so an element that is left out, taken off
   twice or scaled by (sc[j], sc[i]) instead of (sc[i], sc[j]) misses by ten orders of magnitude.  Sizes: every shape the slot dealing distinguishes -- 16 / 19
   the smallest row-per-lane sizes, 31 two tile rows, 64, 67 (K = 10: leading block offset 4, short last panel), 68 a second panel wave, 96 the right-hand-side
   row alone in its tile row, 127 / 131 seven slots per wave, 140 the look-ahead fallback.
2. The mask: what the step never subtracts (above the diagonal, the entry (D, D), tile padding) may hold anything.
3. Whole windows: every launch structure that runs solve_prechain, one step against the extended-precision reference of test_gpu_step.py and a whole solve
   against the oracle and against mode 2 (no chain workgroup: the master eliminates the chain itself and chWW does not exist), twice, bit for bit.
"""
import ctypes as C

import numpy as np
import pytest

import step_ref as sr
from mvil_fusion_amd import abi, lib

pytestmark = pytest.mark.gpu

SIZES = [16, 19, 31, 64, 67, 68, 96, 127, 131, 140]


def _dense_ww(be, A, WW, sc, pad, variant):
    R = A.shape[0]; D = R - 1
    A = np.ascontiguousarray(A, dtype=np.float64); WW = np.ascontiguousarray(WW, dtype=np.float64); sc = np.ascontiguousarray(sc, dtype=np.float64)
    L = np.zeros((R, R)); x = np.zeros(D); ok = C.c_int32(-1)
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    fn = be.lib.vil_debug_dense_solve_ww
    fn.argtypes = [C.c_void_p, C.c_int32, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double), C.c_double, C.POINTER(C.c_double), C.POINTER(C.c_double),
                   C.POINTER(C.c_int32), C.c_int32]
    fn.restype = C.c_int
    assert fn(be.ctx, D, dp(A), dp(WW), dp(sc), float(pad), dp(L), dp(x), C.byref(ok), variant) == 0
    return L, x, ok.value


def _system(D, seed, cond=1e6):
    """M' SPD with condition `cond`, right-hand side y, scales sc, a symmetric WW over all D + 1 rows with |S WW S| ~ |M'|, and A = M' + S WW S (rhs row: y + WW_D S)."""
    rng = np.random.default_rng(seed)
    Q, _ = np.linalg.qr(rng.standard_normal((D, D)))
    M = (Q * np.geomspace(1.0, cond, D)) @ Q.T
    M = 0.5 * (M + M.T)
    y = rng.standard_normal(D) * np.sqrt(cond)
    sc = rng.uniform(0.25, 1.0, D)
    W = rng.standard_normal((D + 1, D + 1)); W = 0.5 * (W + W.T)
    W *= np.abs(M).max() / np.abs(sc[:, None] * W[:D, :D] * sc[None, :]).max()
    A = np.zeros((D + 1, D + 1))
    A[:D, :D] = np.tril(M + sc[:, None] * W[:D, :D] * sc[None, :])
    A[D, :D] = y + W[D, :D] * sc
    return M, y, sc, W, A


@pytest.fixture(scope="module")
def be():
    b = lib.open_vilsolve()
    yield b
    b.close()


@pytest.mark.parametrize("D", SIZES)
def test_subtraction_and_factorisation_against_numpy(be, D):
    M, y, sc, W, A = _system(D, 300 + D)
    Lr = np.linalg.cholesky(M); yr = np.linalg.solve(Lr, y); xr = np.linalg.solve(M, y)
    for variant in (0, 1):
        L, x, ok = _dense_ww(be, A, np.tril(W), sc, 0.0, variant)
        assert ok == 1
        Lf = L[:D, :D]
        back = np.abs(Lf @ Lf.T - M).max() / np.abs(M).max()
        res = np.abs(M @ x - y).max() / (np.abs(M).max() * np.abs(x).max())
        print("D %d variant %d: backward error %.3e |M'|, residual %.3e |M'| |x|" % (D, variant, back, res))
        assert np.allclose(np.triu(Lf, 1), 0.0)
        assert back <= 1e-13
        assert res <= 1e-12
        assert np.abs(Lf - Lr).max() <= 1e-8 * np.abs(Lr).max()
        assert np.abs(L[D, :D] - yr).max() <= 1e-8 * np.abs(yr).max()
        assert np.abs(x - xr).max() <= 1e-8 * np.abs(xr).max()


@pytest.mark.parametrize("D", SIZES)
def test_what_is_masked_never_reaches_the_result(be, D):
    M, y, sc, W, A = _system(D, 700 + D)
    clean = np.tril(W)
    clean[D, D] = 0.0
    bad = clean.copy()
    bad[np.triu_indices(D + 1, 1)] = 1e300
    bad[D, D] = 1e300
    for variant in (0, 1):
        L0, x0, ok0 = _dense_ww(be, A, clean, sc, 0.0, variant)
        L1, x1, ok1 = _dense_ww(be, A, bad, sc, 1e300, variant)
        assert ok0 == 1 and ok1 == 1
        assert np.array_equal(L0, L1) and np.array_equal(x0, x1)


# ---- whole windows: the structures whose master runs solve_prechain (name -> vil_debug_set_launch_mode, launches per iteration it must report) ----------------------------
STRUCTS = {"default": (0, (0, 1)), "mode4": (4, (1,)), "mode3": (3, (2,)), "mode1": (1, (3,))}
KS = (4, 5, 10, 11, 13, 20)


@pytest.fixture(scope="module")
def backends(hip):
    made = {"default": hip}
    for name, mode in (("mode4", 4), ("mode3", 3), ("mode1", 1), ("mode2", 2)):
        b = made[name] = lib.open_vilsolve()
        assert b.lib.vil_debug_set_launch_mode(b.ctx, mode) == 0
    yield made
    for name, b in made.items():
        if name != "default":
            b.close()


@pytest.fixture(scope="module")
def refs(hip, oracle, backends):
    """per K, formed once: the extended-precision step reference, the oracle's solve and mode 2's"""
    cache = {}

    def get(K):
        if K not in cache:
            name = "K%d" % K
            ref = sr.StepRef(hip, sr.make_window(name, oracle), abi.default_options())
            wo = sr.make_window(name, oracle)
            so = oracle.solve(wo, abi.default_options())
            w2 = sr.make_window(name, oracle)
            s2 = backends["mode2"].solve(w2, abi.default_options())
            cache[K] = (ref, so, s2)
        return cache[K]
    return get


def _launches(b):
    lpi, one = C.c_int32(-1), C.c_int32(-1)
    assert b.lib.vil_debug_get_launch_structure(b.ctx, C.byref(lpi), C.byref(one)) == 0
    return lpi.value


@pytest.mark.parametrize("struct", list(STRUCTS))
@pytest.mark.parametrize("K", KS)
def test_one_step_of_every_structure(backends, refs, K, struct):
    b, (ref, _, _) = backends[struct], refs(K)
    step, radius = sr.one_step(b, ref, sr.GN)
    lpi = _launches(b)
    assert lpi in STRUCTS[struct][1], (struct, K, lpi)
    sr.check_step(ref, step, ref.state, sr.GN, radius, lpi < 3, "K%d %s (%d launches)" % (K, struct, lpi))
    again, _ = sr.one_step(b, ref, sr.GN)
    assert np.array_equal(step, again) and np.abs(step).max() > 0


@pytest.mark.parametrize("struct", list(STRUCTS))
@pytest.mark.parametrize("K", KS)
def test_whole_solve_of_every_structure(backends, refs, oracle, K, struct):
    b, (_, so, s2) = backends[struct], refs(K)
    runs = []
    for _ in range(2):
        w = sr.make_window("K%d" % K, oracle)
        sg = b.solve(w, abi.default_options())
        runs.append((sg, w.state_copy()))
    sg, end = runs[0]
    assert abs(sg.initial_cost - so.initial_cost) <= 1e-11 * so.initial_cost
    assert (sg.iterations, sg.successful_steps, sg.termination) == (so.iterations, so.successful_steps, so.termination)
    assert abs(sg.final_cost - so.final_cost) <= 1e-8 * so.final_cost
    n = min(sg.iterations, 64)
    assert np.allclose(np.array(sg.cost_trace[:n]), np.array(so.cost_trace[:n]), rtol=1e-7)
    assert (sg.iterations, sg.successful_steps, sg.termination) == (s2.iterations, s2.successful_steps, s2.termination)      # mode 2: no chWW anywhere
    assert abs(sg.final_cost - s2.final_cost) <= 1e-8 * s2.final_cost
    sh, end_h = runs[1]
    assert (sh.iterations, sh.termination) == (sg.iterations, sg.termination) and sh.final_cost == sg.final_cost
    for k in end:
        assert np.array_equal(end[k], end_h[k], equal_nan=True), k
