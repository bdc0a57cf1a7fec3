"""GPU parity of the voxelised GICP registration (include/vilvgicp.h) against the CPU oracle, through the C-ABI."""
import numpy as np
import pytest

from mvil_fusion_amd import lib, vgicp

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def regs(oracle):
    tx, tc, sx, sc, T_true = vgicp.make_pair(seed=5, rings=16, az=600)
    g = vgicp.Vgicp(lib.load_vilsolve(), "vgicp_"); o = vgicp.Vgicp(oracle.lib, "orc_vgicp_")
    for r in (g, o):
        r.set_target(tx, tc, 0.5); r.set_source(sx, sc)
    yield g, o, T_true
    g.close(); o.close()


@pytest.mark.parametrize("mode", [vgicp.DIRECT1, vgicp.DIRECT7, vgicp.DIRECT27])
def test_linearize_parity(regs, mode):
    g, o, _ = regs
    T = np.eye(4); T[:3, 3] = [0.03, -0.04, 0.01]; T[:3, :3] = vgicp._rot(0.004, -0.003, 0.01)
    eg, Hg, bg, ng = g.linearize(T, mode)
    eo, Ho, bo, no = o.linearize(T, mode)
    assert ng == no and ng > 2000
    assert abs(eg - eo) <= 1e-11 * eo
    assert np.abs(Hg - Ho).max() <= 1e-11 * np.abs(Ho).max() and np.abs(bg - bo).max() <= 1e-10 * np.abs(bo).max()
    eg2, _, _, _ = g.linearize(T, mode, jac=False)
    assert eg2 == eg                                                   # error-only call: same correspondences, same fixed-order sum
    T2 = T.copy(); T2[:3, 3] += [0.01, 0.0, -0.005]
    assert abs(g.compute_error(T2) - o.compute_error(T2)) <= 1e-11 * eo   # stored correspondences, new transform


@pytest.mark.parametrize("optimizer", [vgicp.LM, vgicp.GN])
def test_align_parity(regs, optimizer):
    g, o, T_true = regs
    guess = np.eye(4)
    Tg, sg = g.align(guess, g.default_options(optimizer=optimizer))
    To, so = o.align(guess, o.default_options(optimizer=optimizer))
    assert sg.iterations == so.iterations and sg.converged == so.converged == 1 and sg.n_correspondences == so.n_correspondences
    assert np.abs(Tg - To).max() <= 1e-9
    assert abs(sg.final_error - so.final_error) <= 1e-9 * so.final_error
    assert np.abs(np.array(sg.final_hessian) - np.array(so.final_hessian)).max() <= 1e-9 * np.abs(np.array(so.final_hessian)).max()
    assert np.abs(Tg[:3, 3] - T_true[:3, 3]).max() < 0.03


@pytest.mark.parametrize("case", ["poor_guess", "one_iteration", "two_iterations", "small_lm_budget"])
def test_align_one_pass_per_iteration_paths(regs, case):
    """k_vgicp_align evaluates an LM trial and the NEXT linearisation in one pass and keeps two correspondence caches: rejected trials
    (the speculative linearisation is dropped), loops that end right after an accepted trial (it is never used), and the cache that
    vgicp_error() sees after the alignment must all match the reference flow (linearise, then error passes)."""
    g, o, _ = regs
    guess = np.eye(4)
    kw = {}
    if case == "poor_guess":
        guess[:3, :3] = vgicp._rot(0.05, -0.04, 0.12); guess[:3, 3] = [0.9, -0.7, 0.25]
    elif case == "one_iteration":
        kw = dict(max_iterations=1)
    elif case == "two_iterations":
        kw = dict(max_iterations=2)
    else:
        guess[:3, :3] = vgicp._rot(0.03, 0.02, -0.08); guess[:3, 3] = [-0.6, 0.5, 0.1]
        kw = dict(lm_max_iterations=2, lm_init_lambda_factor=1e-12)
    Tg, sg = g.align(guess, g.default_options(**kw))
    To, so = o.align(guess, o.default_options(**kw))
    assert (sg.iterations, sg.converged, sg.lm_failed, sg.n_correspondences) == (so.iterations, so.converged, so.lm_failed, so.n_correspondences)
    assert np.abs(Tg - To).max() <= 1e-9
    assert abs(sg.final_error - so.final_error) <= 1e-9 * max(so.final_error, 1.0)
    assert np.abs(np.array(sg.final_hessian) - np.array(so.final_hessian)).max() <= 1e-9 * np.abs(np.array(so.final_hessian)).max()
    # the correspondences left behind are those of the last linearisation the loop USED
    T2 = To.copy(); T2[:3, 3] += [0.01, -0.005, 0.002]
    eo = o.compute_error(T2)
    assert abs(g.compute_error(T2) - eo) <= 1e-10 * max(eo, 1.0)


def test_align_repeats_bit_identically(regs):
    """The cooperative kernel's exchange uses relaxed agent-scope atomics and s_waitcnt instead of release / acquire fences, and the
    host polls a sequence number in pinned memory instead of synchronising the stream: 300 back-to-back alignments (alternating guesses,
    so a stale record or a missed partial sum would show) must return the same bits every time."""
    g, _, _ = regs
    g2 = np.eye(4); g2[:3, 3] = [0.05, -0.02, 0.01]
    ref = {}
    for it in range(300):
        k = it & 1
        T, s = g.align(np.eye(4) if k == 0 else g2)
        key = (T.tobytes(), s.iterations, s.n_correspondences, s.final_error)
        if k in ref:
            assert key == ref[k], it
        else:
            ref[k] = key
    assert ref[0][0] != ref[1][0]


def test_errors_and_determinism(regs):
    g, _, _ = regs
    T = np.eye(4)
    a = g.linearize(T)
    b = g.linearize(T)
    assert a[0] == b[0] and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])     # no atomics: bit-reproducible
    with pytest.raises(vgicp.VgicpError):
        g.linearize(T, 5)                                                  # unsupported neighbour mode
    far = np.eye(4); far[:3, 3] = [500.0, 0, 0]
    e, H, bb, n = g.linearize(far)
    assert n == 0 and e == 0.0 and not H.any()                             # no correspondence at all


def test_gpu_reproduces_golden_fixture():
    from test_oracle_vgicp import _check_golden
    g = vgicp.Vgicp(lib.load_vilsolve(), "vgicp_")
    _check_golden(g, vgicp)
    g.close()


def test_covariances_parity(oracle):
    tx, _, sx, _, _ = vgicp.make_pair(seed=9, rings=8, az=400)
    g = vgicp.Vgicp(lib.load_vilsolve(), "vgicp_"); o = vgicp.Vgicp(oracle.lib, "orc_vgicp_")
    for k in (20, 10):
        cg, co = g.covariances(sx, k), o.covariances(sx, k)
        assert np.abs(cg - co).max() < 1e-10                          # same neighbours (exact search, same float distances), same 3 x 3 Jacobi
    small = sx[:7]                                                       # fewer points than k
    assert np.abs(g.covariances(small, 20) - o.covariances(small, 20)).max() < 1e-10
    # covariances estimated inside set_source / set_target: the whole alignment still matches
    for r in (g, o):
        r.set_target(tx, None, 0.5); r.set_source(sx, None)
    Tg, sg = g.align(np.eye(4)); To, so = o.align(np.eye(4))
    assert sg.iterations == so.iterations and sg.converged == so.converged == 1 and np.abs(Tg - To).max() < 1e-8
    g.close(); o.close()


def test_covariances_grid_search_parity(oracle, monkeypatch):
    """The uniform-grid neighbour search (used for clouds >= 4096 points) is exact: forced on a small cloud it reproduces the
    oracle's exhaustive search, for several cell sizes (many rings / exhaustive fallback for isolated points included)."""
    _, _, sx, _, _ = vgicp.make_pair(seed=13, rings=8, az=400)
    sx = np.vstack([sx, np.array([[80.0, -70.0, 30.0], [81.0, -70.5, 30.2]], np.float32)])      # two isolated points far from everything
    o = vgicp.Vgicp(oracle.lib, "orc_vgicp_")
    co = o.covariances(sx, 20)
    import ctypes as C
    for h in (1.0, 0.3, 4.0):
        g = vgicp.Vgicp(lib.load_vilsolve(), "vgicp_")
        assert g.lib.vgicp_set_knn_grid(g.ctx, 0, C.c_double(h)) == 0
        cg = g.covariances(sx, 20)
        g.close()
        assert np.abs(cg - co).max() < 1e-10, h
    o.close()


def test_reuse_across_sources_and_neighbour_modes():
    """One long-lived context against a fresh one at every step, byte for byte, while the source size and the neighbour mode change
    under it: 300 slots fit one workgroup of k_vgicp_align, 1025 x 27 take 55; 257 and 1025 straddle the 256-thread blocks; the
    order grows both correspondence caches, shrinks, then regrows them.  Given covariances, then the brute-force k-NN estimate, then
    the largest source once more through the grid search."""
    import ctypes as C
    from test_gpu_voxelmap import T_SMALL, lin_bytes, same
    tx, tc, sx, sc, _ = vgicp.make_pair(seed=5, rings=4, az=300)
    assert len(tx) == 1200 and len(sx) >= 1025
    so = lib.load_vilsolve()

    def observe(g, mode):
        T, s = g.align(np.eye(4), g.default_options(neighbor_mode=mode))
        summary = (s.iterations, s.converged, s.n_correspondences, s.lm_failed, np.float64(s.final_error).tobytes(), bytes(s.final_hessian))
        return T, summary, np.float64(g.compute_error(T_SMALL)).tobytes(), lin_bytes(g, T_SMALL, mode)      # the error reads the cache the alignment ended in

    steps = [(n, mode, given, False) for given in (True, False) for n, mode in ((300, 1), (1025, 27), (257, 7), (1025, 1), (300, 27))]
    steps.append((1025, 27, False, True))
    used = vgicp.Vgicp(so)
    try:
        used.set_target(tx, tc, 0.5)
        for n, mode, given, grid in steps:
            fresh = vgicp.Vgicp(so)
            try:
                fresh.set_target(tx, tc, 0.5)
                for g in (used, fresh):
                    if grid:
                        assert g.lib.vgicp_set_knn_grid(g.ctx, 0, C.c_double(1.0)) == 0
                    g.set_source(sx[:n], sc[:n] if given else None)
                a, b = observe(used, mode), observe(fresh, mode)
            finally:
                fresh.close()
            assert same(a[0], b[0]) and a[1:] == b[1:], (n, mode, given, grid)
            assert a[1][2] > 0 and a[3][1] > 0, (n, mode, given, grid)          # (correspondences were found: the comparison is not of empty sums)
    finally:
        used.close()


def test_reference_known_answer(oracle):
    """fast_gicp's own registration test data: the GPU passes it, and lands on the oracle's transforms."""
    from test_oracle_vgicp import _kat
    g = vgicp.Vgicp(lib.load_vilsolve(), "vgicp_"); o = vgicp.Vgicp(oracle.lib, "orc_vgicp_")
    Tg, To = _kat(g), _kat(o)
    g.close(); o.close()
    assert np.abs(Tg[0] - To[0]).max() < 1e-8 and np.abs(Tg[1] - To[1]).max() < 1e-8


def test_known_answer_data_all_neighbour_modes(oracle):
    """On the real scans of the reference's own test: GPU and oracle agree for DIRECT7 / DIRECT27 too (linearisation and
    alignment), with the covariances estimated on the device."""
    import os
    d = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "vgicp", "fast_gicp_kat.npz"))
    g = vgicp.Vgicp(lib.load_vilsolve(), "vgicp_"); o = vgicp.Vgicp(oracle.lib, "orc_vgicp_")
    for r in (g, o):
        r.set_target(d["target"], None, 1.0); r.set_source(d["source"], None)
    for mode in (vgicp.DIRECT1, vgicp.DIRECT7, vgicp.DIRECT27):
        eg, Hg, bg, ng = g.linearize(np.eye(4), mode); eo, Ho, bo, no = o.linearize(np.eye(4), mode)
        assert ng == no and abs(eg - eo) <= 1e-10 * eo and np.abs(Hg - Ho).max() <= 1e-10 * np.abs(Ho).max() and np.abs(bg - bo).max() <= 1e-9 * np.abs(bo).max()
    Tg, sg = g.align(np.eye(4), g.default_options(neighbor_mode=vgicp.DIRECT7)); To, so = o.align(np.eye(4), o.default_options(neighbor_mode=vgicp.DIRECT7))
    g.close(); o.close()
    assert sg.iterations == so.iterations and np.abs(Tg - To).max() < 1e-8
