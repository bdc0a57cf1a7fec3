"""imu_sqrtinfo_wg (csrc/vil_eval.hpp: the square-root information U of an IMU record's covariance, pivots through rsqrt plus two Newton steps)
against U = chol(cov^-1)^T in 50-digit arithmetic.

U is not an output of the ABI; it is read out through the whitened Jacobian of vil_eval_factors(FACTOR_IMU), which is U x the raw 15 x 30 Jacobian.
With frame i's quaternion the exact identity the raw (P, p_j) and (V, v_j) blocks are R_i^T = I and the raw (BA, ba_j) and (BG, bg_j) blocks are I
whatever the state, so columns 0:3 of the pose_j block are U[:, 0:3] and columns 0:9 of the speedbias_j block are U[:, 6:15] -- twelve columns of
the device's U with nothing but exact zeros added.  The three rotation columns U[:, 3:6] are NOT read: their raw block is a quaternion product, not
the identity.  The covariances are the device's own records of plain intervals of 3, 5, 24, 60 and 400 samples (lower triangle mirrored, the
triangle the kernel reads); intervals of 1 or 2 samples give covariances numpy's own route fails on, and the estimator never whitens with them.

Measure, per column c: max |U[:, c] - U_ref[:, c]| / max |U_ref[:, c]|.  Floor: that measure for numpy's float64 cholesky(inv(cov)).T, pooled
over the five covariances and the twelve columns.  Bound: 16 x the floor (the margin of tests/test_gpu_posegraph.py).  tests/test_preint_ref.py
holds the oracle's routine to the same measure on all fifteen columns.

Measured on an MI355X (numpy's worst column / the device's worst column, condition number of the covariance):
  3 samples 5.2e-16 / 1.10e-15 (6.7e4)   5 samples 4.6e-16 / 7.5e-16 (2.1e4)   24 samples 5.4e-16 / 5.1e-16 (9.0e2)   60 samples 5.3e-16 / 8.9e-16 (3.4e2)
  400 samples 4.96e-15 / 1.66e-15 (4.6e3)
  pooled floor 4.96e-15, device 1.66e-15: ratio 0.33.  Per covariance the device is at most 2.1 x numpy (3 samples).  What is read out below the
  diagonal is exactly 0 everywhere."""
import numpy as np
import pytest

import preint_ref as pr
from mvil_fusion_amd import abi, lib, preint, synth

pytestmark = pytest.mark.gpu
COLS = [0, 1, 2] + list(range(6, 15))


def device_U(hip, w, cov):
    """the twelve readable columns of the device's U for `cov` in IMU factor 0 of window w (the others come back as 0)"""
    w.imu_const[0, 62:] = cov.ravel()
    _, J = hip.eval_factors(w, abi.FACTOR_IMU)
    J = J.reshape(len(w.imu_i), 480)[0]
    U = np.zeros((15, 15))
    U[:, 0:3] = J[240:345].reshape(15, 7)[:, 0:3]
    U[:, 6:15] = J[345:480].reshape(15, 9)
    return U


def test_sqrt_information_against_50_digits(hip):
    p = preint.Preint(lib.load_vilsolve(), "vpre_")
    rec, _ = p.integrate(*pr.whitening_batch(), want_jacobian=False)
    p.close()
    w = synth.make_config(1)
    w.pose[:, 3:] = [0.0, 0.0, 0.0, 1.0]                                   # R_i = I exactly
    d_np, d_dev = [], []
    for n, r in zip(pr.WHITEN_LENGTHS, rec):
        cov = pr.lower_symmetric(r[62:])
        U = device_U(hip, w, cov)
        assert np.all(np.tril(U, -1) == 0)                                  # what was read out below the diagonal is exactly 0
        U_ref = pr.sqrt_info_mp(cov)
        d_np.append(pr.column_distance(pr.sqrt_info_numpy(cov), U_ref, COLS)); d_dev.append(pr.column_distance(U, U_ref, COLS))
        print("%3d samples, cond %.1e: numpy %.2e, device %.2e (worst column %d)" % (n, np.linalg.cond(cov), d_np[-1].max(), d_dev[-1].max(), COLS[int(np.argmax(d_dev[-1]))]))
    floor = np.max(d_np)
    print("imu_sqrtinfo_wg: floor %.2e, device %.2e, ratio %.2f" % (floor, np.max(d_dev), np.max(d_dev) / floor))
    assert np.max(d_dev) <= 16 * floor
