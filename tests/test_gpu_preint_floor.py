"""k_preint (include/vilpreint.h) against the pre-integration recurrence in 64-bit-mantissa arithmetic (tests/preint_ref.py), per 3 x 3 block.

tests/test_gpu_preint.py compares the kernel with the C++ oracle under max-normalised bounds, which leave the small blocks of the covariance
unresolved (its block maxima span five orders of magnitude) and cannot see the first measurement of an interval.  Here ONE vpre_integrate call
runs the shared fixture of tests/preint_ref.py -- every interval length 0 .. 50 and the batch edges 71 .. 73, 96, 97, fast rotation, zero time
steps with large biases, acc0 / gyr0 independent of the stream; 210 intervals, 6.7 k samples -- and every output of every interval is held to

    distance from the 64-bit-mantissa reference  <=  16 x the float64 floor,

the floor being the distance the float64 sequential recurrence keeps from the same reference, maximised over the fixture; 16 is the margin
tests/test_gpu_posegraph.py gives a device operation order over a float64 floor.  Where the floor is 0 (the blocks that are exactly 0 or I: column
block 0 and the bias rows of J, the (R, BA) and (BA, BG) blocks of P) the device must equal the reference bit for bit.  tests/test_preint_ref.py
proves on the CPU that the kernel's order attains the bound in float64 and that the check rejects five seeded defects.

Measured on an MI355X, floor / the device's distance, each maximised over the 210 intervals (worst interval in brackets):
  J  (P,R) 1.45e-15 / 7.3e-16   (P,V) 5.1e-16 / 1.9e-16   (P,BA) 1.25e-15 / 3.0e-16   (P,BG) 1.50e-15 / 6.2e-16   (R,R) 1.47e-15 / 1.15e-15 [97 plain]
     (R,BG) 1.14e-15 / 4.8e-16   (V,R) 1.38e-15 / 7.3e-16   (V,BA) 9.1e-16 / 4.5e-16   (V,BG) 1.11e-15 / 6.9e-16; the other sixteen blocks bit-equal
  P  (P,P) 3.08e-15 / 6.2e-16   (P,R) 2.19e-15 / 1.51e-15 [97 plain]   (P,V) 2.20e-15 / 6.8e-16   (P,BA) 1.23e-15 / 4.2e-16   (P,BG) 1.38e-15 / 6.0e-16
     (R,R) 1.46e-15 / 1.42e-15 [150 fast]   (R,V) 1.61e-15 / 1.27e-15   (R,BG) 1.33e-15 / 7.0e-16   (V,V) 2.31e-15 / 8.0e-16   (V,BA) 1.31e-15 / 5.5e-16
     (V,BG) 1.57e-15 / 8.2e-16   (BA,BA) 4.9e-16 / 2.7e-16   (BG,BG) 5.5e-16 / 2.7e-16; the transposed blocks alike, (R,BA) and (BA,BG) bit-equal (all 0)
  state  dp 8.7e-16 / 2.7e-16   dq 6.5e-16 / 2.4e-16   dv 9.6e-16 / 2.6e-16   sum_dt 5.1e-16 / 2.0e-16
  worst device / floor ratio 0.97 (P(R,R), 150 samples, fast rotation); with the second noise model 0.45.  The state chain's lane scans and the
  pairwise sums land UNDER the sequential float64 floor; the float64 emulation of the same order (tests/test_preint_ref.py) gives 0.83.
Nothing is above the bound, so no line of the kernel was changed."""
import numpy as np
import pytest

import preint_ref as pr
from mvil_fusion_amd import lib, preint

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    p = preint.Preint(lib.load_vilsolve(), "vpre_")
    yield p
    p.close()


@pytest.fixture(scope="module")
def batch_out(dev):
    """the whole fixture in one launch, with the Jacobian; read-only for every test"""
    rec, jac = dev.integrate(*pr.fixture().batch)
    rec, jac = rec.copy(), jac.copy()
    rec.setflags(write=False); jac.setflags(write=False)
    return rec, jac


def test_every_output_within_16x_the_float64_floor(batch_out):
    fx, (rec, jac) = pr.fixture(), batch_out
    ref = pr.reference(pr.LD)
    ds = [pr.distances(rec[k], jac[k], ref[k]) for k in range(len(fx))]
    lines, worst = pr.report(ds, list(zip(fx.length, fx.variant, fx.seed)))
    print("\n".join(lines)); print("k_preint: worst ratio to the float64 floor %.2f" % worst)
    bad = [(fx.length[k], fx.variant[k], fx.seed[k]) + v for k in range(len(fx)) for v in pr.violations(rec[k], jac[k], ref[k])]
    assert bad == []


def test_exact_structure(dev, batch_out):
    fx, (rec, jac) = pr.fixture(), batch_out
    start, dt, acc, gyr, acc0, gyr0, ba, bg = fx.batch
    for off, (r0, c0) in zip((17, 26, 35, 44, 53), ((0, 9), (0, 12), (3, 12), (6, 9), (6, 12))):        # the record's five blocks ARE the Jacobian's
        assert np.array_equal(rec[:, off:off + 9].reshape(-1, 3, 3), jac[:, r0:r0 + 3, c0:c0 + 3])
    assert np.array_equal(rec[:, 10:13], ba) and np.array_equal(rec[:, 13:16], bg)
    for k in (k for k in range(len(fx)) if fx.length[k] == 0):                                          # an empty interval: the identity record
        assert np.array_equal(rec[k, :10], [0, 0, 0, 0, 0, 0, 1, 0, 0, 0]) and rec[k, 16] == 0
        assert np.all(rec[k, 17:62] == 0) and np.all(rec[k, 62:] == 0) and np.array_equal(jac[k], np.eye(15))
    rec2, none = dev.integrate(*fx.batch, want_jacobian=False)                                          # without the Jacobian output: the same bits
    assert none is None and np.array_equal(rec2, rec)


def test_intervals_do_not_depend_on_their_neighbours(dev, batch_out):
    fx, (rec, jac) = pr.fixture(), batch_out
    for n in (1, 12, 23, 24, 25, 48, 49, 97):                                                           # alone (n = 1) as in the batch
        k = fx.find(n, "plain", 1)
        r1, j1 = dev.integrate(*fx.subset([k]))
        assert np.array_equal(r1[0], rec[k]) and np.array_equal(j1[0], jac[k]), n
    order = list(range(len(fx)))[::-1]
    rr, jr = dev.integrate(*fx.subset(order))                                                           # the batch reversed
    assert np.array_equal(rr, rec[order]) and np.array_equal(jr, jac[order])


def test_another_noise_model(dev):
    """the plain lengths 7, 24, 49 with four noise densities that differ from preint.NOISE and from one another by factors that are no powers of two"""
    fx = pr.fixture()
    noise = (pr.NOISE[0] * 3.0, pr.NOISE[0] * 0.7, pr.NOISE[0] * 0.11, pr.NOISE[0] * 0.013)
    ks = tuple(fx.find(n, "plain", s) for s in pr.SEEDS for n in (7, 24, 49))
    rec, jac = dev.integrate(*fx.subset(ks), noise=np.array(noise))
    ref = pr.reference(pr.LD, noise, ks)
    ds = [pr.distances(rec[i], jac[i], ref[i]) for i in range(len(ks))]
    lines, worst = pr.report(ds, [(fx.length[k], fx.variant[k], fx.seed[k]) for k in ks])
    print("\n".join(l for l in lines if l.startswith("P("))); print("k_preint, second noise model: worst ratio to the float64 floor %.2f" % worst)
    assert [v for i in range(len(ks)) for v in pr.violations(rec[i], jac[i], ref[i])] == []
    base = pr.reference(pr.LD)
    assert all(np.abs(np.asarray(ref[i][5] - base[k][5], np.float64)).max() > 0.1 * np.abs(np.asarray(base[k][5], np.float64)).max() for i, k in enumerate(ks))   # really another P
