"""vil_eval_factors and vil_eval_lidar_functors against the 50-digit dual-number reference of tests/factors_ref.py, per factor and per block.

The suite's precision claims rest on vil_eval_factors (tests/test_gpu_step.py and tests/test_gpu_marg.py assemble their extended-precision systems from
it), and the device functions behind it -- visual_eval, plane_eval, edge_eval, imu_common / imu_block, icp_eval1, lps_eval1, prior_block_dx of
csrc/vil_factors.hpp -- are the ones the sweep calls.  tests/test_gpu_parity.py holds them to the C++ oracle under one norm-wise 1e-12 per class on an
ordinary window; the oracle was written from the same condensed formulas and its Jacobians are pinned by finite differences at 2e-6.  Here every
residual and every Jacobian block of every factor of the fixture (visual: inverse depth 1e-3 and 10, z = 0.1, image corner, td with 5 /s velocities and
rolling-shutter rows, use_td = 0, 120 degrees between frames, qw < 0; IMU: dbg 0 / 1e-3 / 5e-2 with dba 0.5, sum_dt 0.005 and 1, rotation residual 0
and 170 degrees, negative-w quaternions; ICP / LPS: both slerp branches, bracket angles 1e-6 .. 3 rad, flips, t at and next to its ends; LiDAR points
0.3 m and 150 m away, |a - b| 1e-3 and 50, points on the line / plane, a sliver triangle; the prior with every block kind, sign flips, |dx| 1e-9 and
0.5) is held to

    distance from the 50-digit reference  <=  16 x max(float64 floor, 2^-52),      bit-equal where the floor is 0,

the floor being the distance of the float64 dual evaluation from the same reference, per class, case family and block position.  The reference
differentiates the residual as the reference sources write it; where the reference's analytic Jacobian is not that derivative
(factors_ref.DEVIATIONS: the IMU rotation rows at dbg != 0, the prior's stored Jacobian) the reference value is its own formula in 50 digits.
tests/test_factors_ref.py proves the instrument on the CPU: the oracle passes it, eight seeded defects do not.

Measured on an MI355X (float64 floor, the largest over the capped families / the device's distance at its worst ratio / that ratio, worst case named):
  IMU, whitened, 3 x 3 blocks: floors 3.2e-16 .. 3.5e-15, (P,bg_i) 5.4e-13 and (P,bg_j) 4.7e-13 (small blocks of U: the covariance's conditioning);
       worst (V,bg_i) 2.6e-15 / 1.2e-15 / 5.49 [dbg 1e-3, dba 0.5]; (P,ba_i) 4.26 [rot 0]; (P,bg_j) 4.01 [rot 0]; residuals 0.6 .. 1.8; the 21 blocks below
       U's diagonal and both columns 7 bit-equal
  visual: r 4.7e-14 / 2.3e-15 / 1.47   pose_i 8.9e-14 / 8.7e-14 / 4.13 [z_j = 0.1]   pose_j 8.9e-14 / 8.7e-14 / 1.67   ex 1.5e-13 / 8.7e-14 / 4.07
       inverse depth 1.9e-13 / 1.8e-14 / 1.49 [lam = 10]   td 4.1e-14 / 7.8e-14 / 1.89; columns 7 and the td block of use_td = 0 bit-equal
  prior: r 1.4e-15 / 1.9e-15 / 1.39 [|dx| = 1e-9, no flip]; the Jacobian bit-equal to the stored matrix
  ICP: r 9.8e-16 / 5.3e-16 / 2.39; pose blocks 8.5e-15 .. 1.7e-14 / 2.2e-16 .. 1.2e-15 / 1.32 [th = 3 | identical]; row 1 bit-equal
  LPS: r 9.9e-17 / 6.2e-17 / 0.28; pose blocks 6.0e-14, 1.1e-13 / 1.1e-13 / 1.03 [th = 1e-2, t = 0.5]
  edge: r 9.2e-16 / 5.2e-16 / 1.08, J 1.3e-14 / 7.2e-16 / 1.39     plane: r 1.1e-15 / 1.9e-15 / 3.42 [150 m, qw < 0], J 2.1e-15 / 1.5e-15 / 1.37
  functors: edge 2.63 [150 m], PLANE3 2.63 (floor 7.6e-14: the sliver), plane-norm 3.05 [150 m], distance 2.19 [150 m]; columns 7 bit-equal
  worst ratio over everything capped: 5.49.
ICP / LPS families are (bracket angle, class of t); in ICP the a / b blocks carry the first bracket's family, c / d the second's.  Capped (floor under
1e-12): identical, th = 1 and th = 3 with t in {0, 0.5, 1}, in LPS also th = 1e-2 (floor 6.0e-14 / 1.1e-13, device 1.1e-13, ratio 1.03).
Reported only (factors_ref.REPORTED_ONLY, each bounded by 16 x its OWN floor; float64 floors of eps / th^2 and eps / t that belong to the reference's
formula, not to the fixture), floor of pose a, pose b / the device's worst ratio:
  th = 1e-3, t in {0, 0.5, 1}: LPS 9.6e-12, 1.4e-11 / 0.76   ICP 3.0e-10, 4.5e-10 / 0.76        th = 1e-2, t in {0, 0.5, 1}, ICP: 1.6e-12, 2.9e-12 / 1.03
  t = 1e-9 (pose b small) and 1 - 1e-9 (pose a small), that block: th = 1 3.2e-09 .. 3.6e-07, th = 3 2.6e-07 .. 2.0e-05, th = 1e-2 2.7e-05 .. 2.9e-03,
  th = 1e-3 3.7e-03 .. 0.25; the other block of such a factor stays at its angle's floor; worst ratio over these families 2.59
  th = 1e-6, one floor per class over the pose blocks: LPS 6.7e+03, ICP 3.8e+05 / 1.3
csrc/vil_factors.hpp meets the bound as it is.  Functor kinds 0 and 2 equal the window's EDGE and PLANE classes bit for bit because k_eval_lidar and
k_eval_lidar_functors call one out-of-line lidar_point_eval (csrc/vil_eval.hpp): inlined into each kernel, quatR / edge_eval / plane_eval are contracted
into different fused multiply-adds and the two differ by up to 3e-13 of the residual's size at six poses of ten."""
import numpy as np
import pytest

import factors_ref as fr

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def device_out(hip):
    """every case of every class through the device once, with Jacobians; read-only for the tests"""
    out = {}
    for key in fr.KEYS:
        out[key] = []
        for case in fr.fixture(key):
            r, J = fr.backend_eval(hip, case)
            r.setflags(write=False); J.setflags(write=False)
            out[key].append((r, J))
    return out


@pytest.mark.parametrize("key", fr.KEYS)
def test_every_block_within_16x_the_float64_floor(device_out, key):
    results, bad = [], []
    for case, ref, (r, J) in zip(fr.fixture(key), fr.reference(key), device_out[key]):
        results.append((case, fr.distances(case, r, J, ref)))
        bad += fr.violations(case, r, J, ref)
    lines, worst, worst_ro = fr.report(key, results)
    print("\n".join(lines)); print("device, %s: worst ratio to the float64 floor %.2f (reported-only families %.2f)" % (key, worst, worst_ro))
    assert bad == []


@pytest.mark.parametrize("key", fr.KEYS)
def test_residuals_alone_are_the_same_bits(hip, device_out, key):
    for case, (r, _) in zip(fr.fixture(key), device_out[key]):
        r2, none = fr.backend_eval(hip, case, jac=False)
        assert none is None and np.array_equal(r2, r), case.name


@pytest.mark.parametrize("key", [k for k in fr.KEYS if k != "prior"])
def test_a_factor_does_not_depend_on_its_neighbours(hip, device_out, key):
    """the fixture's factors reversed, and one factor alone, give the same bits"""
    for case, (r, J) in zip(fr.fixture(key), device_out[key]):
        order = list(range(case.nfactors))[::-1]
        rr, Jr = fr.backend_eval(hip, fr.subcase(case, order))
        assert np.array_equal(rr, r[order]) and np.array_equal(Jr, J[order]), case.name
        for f in (0, case.nfactors // 2, case.nfactors - 1):
            r1, J1 = fr.backend_eval(hip, fr.subcase(case, [f]))
            assert np.array_equal(r1[0], r[f]) and np.array_equal(J1[0], J[f]), (case.name, f)


def test_functor_kinds_0_and_2_equal_the_window_classes(hip, device_out):
    """the device twin of test_oracle_factors.py::test_edge_and_plane_norm_functor_batches_equal_the_window_classes"""
    for key, kind in (("edge", 0), ("plane", 2)):
        for case, (r, J) in zip(fr.fixture(key), device_out[key]):
            w = case.w
            pose_of, consts = (w.edge_pose, w.edge_const) if kind == 0 else (w.plane_pose, w.plane_const)
            for k in range(w.K):                     # every pose: which quaternions two differently contracted kernels disagree on is not predictable
                m = pose_of == k
                assert m.any()
                rf, Jf = fr.eval_functors(hip, kind, consts[m], w.q_lb, w.t_lb, w.pose[k])
                assert np.array_equal(rf, r[m]) and np.array_equal(Jf, J[m]), (key, case.name, k)
