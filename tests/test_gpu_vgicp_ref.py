"""The device's voxelised GICP registration (include/vilvgicp.h, csrc/vilvgicp.hip) against the 50-digit restatement of fast_gicp
(tests/vgicp_ref.py) on the fixtures of tests/vgicp_fixtures.py.  tests/test_vgicp_ref.py runs the oracle and twelve deliberate mistakes
through the same judge on the CPU.

Bounds -- none comes from the device's output:
  counts, flags, iterations     equal to the restatement's.
  vgicp_linearize               per quantity (err | b rotation | b translation | H rr | H rt | H tt): the largest absolute distance from the
                                50-digit values is at most MARGIN = 16 x floor, floor = the largest such distance of the float64 route of the
                                restatement, summed in ascending and in descending slot order (vgicp_ref.F64_ROUTES; the reference's OpenMP
                                reduction fixes no order), on the same inputs; floor > 0 is asserted.  With and without H / b; edges on the
                                error alone, and with H / b at res 0.1.
  vgicp_compute_error           at a second transform, on the correspondences of the linearisation: 16 x the float64 floor of that error.
  vgicp_covariances             per point 16 x the fixture's float64 floor, clamped below at 8 ulp of 1; lattice: diag(.., 1e-3, ..) to 8 ulp.
                                Degenerate clouds: finite, symmetric to 1 ulp, trace 2.001 to 4 ulp, eigenvalues (1e-3, 1, 1) to 1e-12.
  vgicp_align                   T, final_error, final_hessian within 16 x their floors (float64 loop against 50-digit loop); the floor of T is
                                clamped below at iterations x 2^-52 x (1 + max |t|), the rounding of the state at each composition.
  two_slots                     k_vgicp_align against vgicp_linearize (held to 50 digits above) at the same transform, a reordered sum of n
                                terms: |d err| <= 2 n 2^-53 err (non-negative terms), |d H_pq| <= 2 n 2^-53 sqrt(H_pp H_qq) (positive
                                semi-definite summands); iterations, flags and T against the oracle as tests/test_gpu_vgicp.py.

Measured on an MI355X: MEASURED below holds the largest distance / floor ratio per family and quantity (`align`: over the seven cases; the
figures are printed by `pytest -s`), docs/vgicp.md the whole table.  With vd::rcp_nr in inv3, edges (res 0.1, axis y, k 41, DIRECT1)
measures 8.36e-16 against a floor of 5.17e-17: ratio 16.2.  The 50-digit values of all fixtures take about 20 s on one
core, once per process."""
import ctypes as C

import numpy as np
import pytest

import vgicp_fixtures as fx
import vgicp_ref as ref
from mvil_fusion_amd import lib, vgicp

pytestmark = pytest.mark.gpu

MEASURED = """
family                   quantity       distance   floor      ratio
edges                    err            1.00e-15   1.14e-16   8.77
edges                    b_rot          2.98e-15   2.74e-15   1.09
edges                    b_trans        1.68e-14   5.45e-15   3.08
edges                    H_rr           4.03e-05   3.23e-05   1.25
edges                    H_rt           1.04e-13   6.16e-13   0.17
edges                    H_tt           1.15e-12   7.19e-12   0.16
offsets                  err            8.51e-14   8.51e-14   1.00
offsets                  b_rot          9.11e-13   4.56e-13   2.00
offsets                  b_trans        1.51e-13   1.23e-13   1.23
offsets                  H_rr           8.41e-12   8.27e-12   1.02
offsets                  H_rt           2.24e-12   2.46e-12   0.91
offsets                  H_tt           5.25e-13   7.52e-13   0.70
offsets compute_error    err            5.24e-14   5.95e-14   0.88
blocks                   err            4.53e-14   3.91e-14   1.16
blocks                   b_rot          1.79e-14   1.25e-14   1.43
blocks                   b_trans        2.82e-12   2.17e-12   1.30
blocks                   H_rr           4.83e-14   4.83e-14   1.00
blocks                   H_rt           3.55e-14   3.02e-14   1.18
blocks                   H_tt           1.37e-14   4.13e-15   3.32
blocks compute_error     err            4.66e-14   4.04e-14   1.15
cov lattice              C              0.00e+00   1.78e-15   0.00
cov tie                  C              4.91e-16   1.78e-15   0.28
cov tie_swapped          C              4.91e-16   1.78e-15   0.28
cov unfused              C              3.53e-16   1.78e-15   0.20
cov tilted               C              4.62e-15   5.51e-15   0.84
align                    T              1.29e-14   1.25e-14   1.03
align                    final_error    3.38e-15   3.72e-15   0.91
align                    final_hessian  8.39e-11   1.64e-10   0.51
align                    compute_error  5.46e-15   5.46e-15   1.00
"""

BUILDERS = {"host": vgicp.BUILD_HOST, "device": vgicp.BUILD_DEVICE}


@pytest.fixture(params=list(BUILDERS))
def gpu(request):
    g = vgicp.Vgicp(lib.load_vilsolve(), "vgicp_")
    g.set_voxel_builder(BUILDERS[request.param])
    yield g
    g.close()


@pytest.fixture()
def gpu1():
    g = vgicp.Vgicp(lib.load_vilsolve(), "vgicp_")
    yield g
    g.close()


@pytest.mark.parametrize("res", fx.EDGE_RES)
def test_edges(gpu, res):
    """vox_coord: transformed coordinates on a cell edge and up to 64 doubles either side of it, where x * (1 / res) and x / res disagree."""
    for axis in range(3):
        for k in fx.EDGE_K:
            P, T = fx.edges(axis, res, k)
            fx.load(gpu, P)
            for mode in fx.MODES:
                fx.judge_linearize(gpu, P, T, mode, want_H=False, tag="edges:%g/%d/%d/%d" % (res, axis, k, mode))
                if res == fx.EDGE_RES_WITH_H:
                    fx.judge_linearize(gpu, P, T, mode, tag="edges:%g/%d/%d/%d/H" % (res, axis, k, mode))


def test_offsets_and_far(gpu):
    """The DIRECT7 / DIRECT27 offset decoding, one cluster per offset; a voxel coordinate beyond the 21 bits of the key finds nothing."""
    P, T, _ = fx.offsets_fixture()
    fx.load(gpu, P)
    for mode in fx.MODES:
        fx.judge_linearize(gpu, P, T, mode, second=True, tag="offsets:%d" % mode)
    P, T = fx.far()
    fx.load(gpu, P)
    for mode in fx.MODES:
        fx.judge_linearize(gpu, P, T, mode, tag="far:%d" % mode)


@pytest.mark.parametrize("name", [c[0] for c in fx.BLOCK_CASES])
def test_blocks(gpu, name):
    """inv3, the per-slot sums, block_fold + k_vgicp_sum: sizes either side of the 256-thread block and of k_vgicp_align's 512."""
    P, T, mode = fx.blocks(name)
    fx.load(gpu, P)
    fx.judge_linearize(gpu, P, T, mode, second=True, tag="blocks:" + name)
    fx.judge_linearize(gpu, P, T, mode, want_H=False, tag="blocks:" + name + "/err")


SEARCHES = {"exhaustive": None, "grid1.0": 1.0, "grid0.3": 0.3, "grid4.0": 4.0}


def _search(g, how):
    if SEARCHES[how] is not None:
        assert g.lib.vgicp_set_knn_grid(g.ctx, 0, C.c_double(SEARCHES[how])) == 0


@pytest.mark.parametrize("how", list(SEARCHES))
@pytest.mark.parametrize("name", list(fx.COV_CLOUDS))
def test_covariances(gpu1, name, how):
    _search(gpu1, how)
    got = gpu1.covariances(fx.COV_CLOUDS[name](), fx.K)
    ok, d, fl = fx.judge_cov(got, name)
    print("vgicp-ref cov", name, how, "%.2e/%.2e" % (d, fl))
    assert ok, (d, fl)
    if name == "lattice":
        axes = fx.lattice()[1]
        want = np.array([np.diag([1e-3 if r == a else 1.0 for r in range(3)]) for a in axes]).reshape(-1, 9)
        assert np.abs(got - want).max() <= 8 * fx.ULP


@pytest.mark.parametrize("how", list(SEARCHES))
@pytest.mark.parametrize("kind", ["collinear", "coincident"])
def test_degenerate(gpu1, kind, how):
    _search(gpu1, how)
    fx.check_degenerate(gpu1.covariances(fx.degenerate(kind), fx.K))


@pytest.mark.parametrize("name", list(fx.ALIGN_CASES))
def test_align(gpu1, name):
    P, guess, opts = fx.align_case(name)
    fx.load(gpu1, P)
    T, s = gpu1.align(guess, gpu1.default_options(**opts))
    ok, v = fx.judge_align(fx.summary_from(T, s), name)
    print("vgicp-ref align", name, v)
    assert ok, v
    # the correspondences left behind are those of the last linearisation the loop USED
    m, f = fx.aligned(name, "mp"), fx.aligned(name, "f64")
    T2 = fx.second_transform(ref.to_np(m["T"]))
    want = ref.compute_error(P, T2, m["lin"], ref.MP)
    floor = abs(float(ref.compute_error(P, T2, f["lin"], ref.F64) - want))
    d = abs(float(ref.mp.mpf(gpu1.compute_error(T2)) - want))
    print("vgicp-ref align", name, "err2 %.2e/%.2e" % (d, floor))
    assert floor > 0 and d <= ref.MARGIN * floor


@pytest.mark.parametrize("optimizer,iterations", [(vgicp.GN, 1), (vgicp.LM, 2)])
def test_two_slots(gpu1, oracle, optimizer, iterations):
    """65 610 slots: threads of k_vgicp_align take a second slot in the grid-stride loop."""
    tx, tc, sx, sc, T0 = fx.two_slots()
    o = vgicp.Vgicp(oracle.lib, "orc_vgicp_")
    try:
        for r in (gpu1, o):
            r.set_target(tx, tc, 0.5); r.set_source(sx, sc)
        kw = dict(neighbor_mode=27, optimizer=optimizer, max_iterations=iterations)
        Tg, sg = gpu1.align(T0, gpu1.default_options(**kw))
        To, so = o.align(T0, o.default_options(**kw))
    finally:
        o.close()
    assert (sg.iterations, sg.converged, sg.lm_failed, sg.n_correspondences) == (so.iterations, so.converged, so.lm_failed, so.n_correspondences)
    assert np.abs(Tg - To).max() <= 1e-9
    # the last linearisation of the loop: at the guess (one iteration) or at the transform the first iteration stepped to (it was accepted)
    if iterations == 1:
        T_lin = T0
    else:
        T1, s1 = gpu1.align(T0, gpu1.default_options(**dict(kw, max_iterations=1)))
        assert s1.iterations == 1 and np.abs(T1 - T0).max() > 0
        T_lin = T1
        Tg, sg = gpu1.align(T0, gpu1.default_options(**kw))
    e, H, b, n = gpu1.linearize(T_lin, 27)
    assert n == sg.n_correspondences and n > 30000
    u = 2 * n * 2.0 ** -53
    assert abs(sg.final_error - e) <= u * e
    Hs = np.array(sg.final_hessian).reshape(6, 6)
    dg = np.sqrt(np.diag(H))
    assert (np.abs(Hs - H) <= u * np.outer(dg, dg)).all()
