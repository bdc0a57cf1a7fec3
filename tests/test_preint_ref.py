"""Proves the instrument of tests/test_gpu_preint_floor.py and tests/test_gpu_imu_whitening.py on the CPU (tests/preint_ref.py).

  * the new float64 reference agrees with the two existing restatements of the recurrence (synth.preintegrate, orc_vpre_integrate) to 16 x the
    float64 floor per block, bit for bit where that floor is 0;
  * the kernel's documented order (batches of 24, pairwise tree, fold), restated in float64, stays within the GPU test's bound on the whole
    fixture, so the bound is attainable;
  * the GPU test's checking function rejects five seeded defects;
  * the oracle's square-root information is held to the measure the device is held to.

Measured (float64 floor = float64 sequential against 64-bit-mantissa sequential, pooled over the 210 intervals of the fixture; per block 4.9e-16 ..
3.1e-15, the state 5.1e-16 .. 9.6e-16, listed in tests/test_gpu_preint_floor.py):
  tree order, state chain sample by sample: worst ratio to the floor 1.13 (J(V,BA), 150 samples, fast rotation)
  tree order, state chain by the kernel's lane scans: worst ratio 0.83 (P(R,R)); every block that is exactly 0 or I in the reference is bit-equal
  oracle's square-root information: worst column 4.8e-15 against numpy's 3.3e-15 (ratio 1.46); E = max |U cov U^T - I| per covariance (3, 5, 24, 60,
  400 samples) numpy 3.2e-15, 8.2e-16, 1.3e-15, 9.2e-16, 1.6e-14, oracle 1.7e-15, 4.0e-15, 1.2e-15, 2.4e-15, 1.8e-14
Seeded defects on the 30-sample plain interval of seed 0 (old bound: max |P - P_ref| <= 1e-12 x max |P_ref|, the metric of tests/test_gpu_preint.py):
  (a) Q_b of pair 0 left out at the st = 4 level of the first batch: max |dP| / max |P| = 1.4e-1.  The old bound SEES this one -- slot 4 holds four
      samples' noise, a seventh of the (V, V) block --, so a dropped Q_b was never among what the old metric let through; the new check fails it
      in 21 blocks of P.
  (c) the (P, BG) block x (1 + 1e-10): max |dP| / max |P| = 4.5e-16, far under the old 1e-12, so the old bound passes it (asserted below); the new
      check fails it at 7.2e4 x the floor.
"""
import numpy as np
import pytest

import preint_ref as pr
from mvil_fusion_amd import preint, synth


def test_constants_match_the_package():
    assert tuple(preint.NOISE) == pr.NOISE and pr.NOISE == (synth.ACC_N, synth.GYR_N, synth.ACC_W, synth.GYR_W)


def test_fixture_contents():
    fx = pr.fixture()
    plain = {(l, s) for l, v, s in zip(fx.length, fx.variant, fx.seed) if v == "plain"}
    assert plain == {(l, s) for l in list(range(51)) + [71, 72, 73, 96, 97] for s in pr.SEEDS}
    for var in ("fast", "degenerate"):
        assert sorted(l for l, v, s in zip(fx.length, fx.variant, fx.seed) if v == var and s == 0) == [1, 7, 23, 24, 25, 49, 150]
    start, dt, acc, gyr, acc0, gyr0, ba, bg = fx.batch
    # every tail size 1 .. 24 occurs, and both sides of every batch edge
    assert {l % pr.PRE_B or pr.PRE_B for l in fx.length if l} == set(range(1, 25)) and {24, 25, 48, 49, 72, 73} <= set(fx.length)
    # the first measurement of an interval is not the sample before it
    for k in range(1, len(fx)):
        if start[k] > 0:
            assert not np.array_equal(acc0[k], acc[start[k] - 1]) and not np.array_equal(gyr0[k], gyr[start[k] - 1])
    k = fx.find(25, "degenerate")
    assert np.count_nonzero(dt[start[k]:start[k + 1]] == 0) == 5
    # which tail sizes take the wide path of the tree (k_preint: pairs x 50 tasks >= 256 lanes)
    assert [nb for nb in range(1, 25) if pr.tree_levels(nb) and pr.tree_levels(nb)[0][2]] == list(range(12, 25))
    assert [nb for nb in range(1, 25) if len(pr.tree_levels(nb)) > 1 and pr.tree_levels(nb)[1][2]] == [23, 24]
    assert not any(w for nb in range(1, 25) for st, _, w in pr.tree_levels(nb) if st >= 4)


def _jac_from_record(rec, J):
    """synth.preintegrate returns the record alone: its five Jacobian blocks placed into a copy of J"""
    J = np.array(J, np.float64)
    for off, (r0, c0) in zip((17, 26, 35, 44, 53), ((0, 9), (0, 12), (3, 12), (6, 9), (6, 12))):
        J[r0:r0 + 3, c0:c0 + 3] = rec[off:off + 9].reshape(3, 3)
    return J


def test_float64_reference_equals_the_existing_restatements(oracle):
    fx = pr.fixture()
    o = preint.Preint(oracle.lib, "orc_vpre_")
    ro, jo = o.integrate(*fx.batch)
    o.close()
    ref64 = pr.reference(np.float64)
    for k in range(len(fx)):
        assert pr.violations(ro[k], jo[k], ref64[k]) == [], ("oracle", fx.length[k], fx.variant[k], fx.seed[k])
        assert np.array_equal(ro[k][10:16], np.concatenate([fx.batch[6][k], fx.batch[7][k]]))
    for k in range(0, len(fx), 3):                                       # synth.preintegrate is a Python loop: every third interval
        rs = synth.preintegrate(*fx.interval(k))
        assert pr.violations(rs, _jac_from_record(rs, ref64[k][4]), ref64[k]) == [], ("synth", fx.length[k], fx.variant[k], fx.seed[k])


@pytest.mark.parametrize("scans", [False, True])
def test_tree_emulation_stays_within_the_gpu_bound(scans):
    """The bound of the GPU test is attainable by the kernel's order in float64 -- with the state chain sample by sample (the tree alone) and
    with the chain by the kernel's prefix product and prefix sums."""
    fx = pr.fixture()
    ref = pr.reference(pr.LD)
    ds, bad = [], []
    for k in range(len(fx)):
        rec, jac = pr.to_record(pr.tree_emulation(*fx.interval(k), pr.NOISE, scans=scans), fx.batch[6][k], fx.batch[7][k])
        ds.append(pr.distances(rec, jac, ref[k]))
        bad += [(fx.length[k], fx.variant[k], fx.seed[k]) + v for v in pr.violations(rec, jac, ref[k])]
    lines, worst = pr.report(ds, list(zip(fx.length, fx.variant, fx.seed)))
    print("\n".join(lines)); print("tree emulation (scans=%s): worst ratio to the floor %.2f" % (scans, worst))
    assert bad == []


def test_the_check_rejects_seeded_errors():
    """Each of these records comes from the emulation on the 30-sample plain interval of seed 0 and must fail pr.violations, the function the GPU
    test asserts with; the unmodified emulation passes.  (a) and (c) are also put to the old bound, see the module docstring."""
    fx = pr.fixture()
    k = fx.find(30)
    assert k > 0 and fx.batch[0][k] > 0
    ref = pr.reference(pr.LD)[k]
    args, ba, bg = fx.interval(k), fx.batch[6][k], fx.batch[7][k]
    good, good_j = pr.to_record(pr.tree_emulation(*args, pr.NOISE), ba, bg)
    assert pr.violations(good, good_j, ref) == []
    P_ref = np.asarray(ref[5], np.float64)
    old = lambda rec: np.abs(rec[62:].reshape(15, 15) - P_ref).max() / np.abs(P_ref).max()
    names = lambda v: {x[0] for x in v}

    # (a) Q_b of one pair left out at the st = 4 level
    rec, jac = pr.to_record(pr.tree_emulation(*args, pr.NOISE, defect=("drop_qb", 4, 0)), ba, bg)
    va = pr.violations(rec, jac, ref)
    print("(a) old metric %.2e, new violations %d, worst %.1e x floor" % (old(rec), len(va), max(d / f for _, d, f in va if f > 0)))
    assert va and all(n.startswith("P(") for n in names(va)) and old(rec) > 1e-12       # (the old bound rejects this one as well)
    # (b) the first sample integrated from the previous interval's last sample
    s0 = fx.batch[0][k]
    wrong = list(args); wrong[3], wrong[4] = fx.batch[2][s0 - 1], fx.batch[3][s0 - 1]
    rec, jac = pr.to_record(pr.tree_emulation(*wrong, pr.NOISE), ba, bg)
    assert {"dp", "dv", "dq"} <= names(pr.violations(rec, jac, ref))
    # (c) the (P, BG) block of P x (1 + 1e-10)
    rec = good.copy(); P = rec[62:].reshape(15, 15); P[0:3, 12:15] *= 1 + 1e-10
    vc = pr.violations(rec, good_j, ref)
    print("(c) old metric %.2e, new %.1e x floor" % (old(rec), vc[0][1] / vc[0][2]))
    assert names(vc) == {"P(P,BG)"} and old(rec) <= 1e-12                # the old bound lets it through
    # (d) Rr from the normalised product
    rec, jac = pr.to_record(pr.tree_emulation(*args, pr.NOISE, defect=("rr_normalised",)), ba, bg)
    assert pr.violations(rec, jac, ref)
    # (e) one entry of J's bias rows set to 1e-300
    jac = good_j.copy(); jac[10, 4] = 1e-300
    assert names(pr.violations(good, jac, ref)) == {"J(BA,R)"}


# ---- the square-root information ---------------------------------------------------------------------------------------------------------------------
def test_oracle_sqrt_info_against_50_digits(oracle):
    """orc_imu_sqrt_info on the covariances of plain intervals of 3, 5, 24, 60 and 400 samples: every column of U within 16 x the distance numpy's
    float64 cholesky(inv(cov)).T keeps from the 50-digit U (pooled over covariances and columns), and E = max |U cov U^T - I| within 16 x numpy's."""
    import ctypes as C
    o = preint.Preint(oracle.lib, "orc_vpre_")
    rec, _ = o.integrate(*pr.whitening_batch(), want_jacobian=False)
    o.close()
    f = oracle.lib.orc_imu_sqrt_info
    f.restype = C.c_int
    dp = C.POINTER(C.c_double)
    d_np, d_orc, e_np, e_orc = [], [], [], []
    for r in rec:
        cov = pr.lower_symmetric(r[62:])
        U = np.zeros((15, 15))
        assert f(cov.ctypes.data_as(dp), U.ctypes.data_as(dp)) == 0
        assert np.all(np.tril(U, -1) == 0)
        U_ref = pr.sqrt_info_mp(cov)
        d_np.append(pr.column_distance(pr.sqrt_info_numpy(cov), U_ref, range(15))); d_orc.append(pr.column_distance(U, U_ref, range(15)))
        e_np.append(pr.whitening_error(pr.sqrt_info_numpy(cov), cov)); e_orc.append(pr.whitening_error(U, cov))
    floor = np.max(d_np)
    print("columns: numpy floor %.2e, oracle %.2e (ratio %.2f); E: numpy %s, oracle %s" % (floor, np.max(d_orc), np.max(d_orc) / floor, ["%.1e" % e for e in e_np], ["%.1e" % e for e in e_orc]))
    assert np.max(d_orc) <= 16 * floor
    assert all(eo <= 16 * en for eo, en in zip(e_orc, e_np))
