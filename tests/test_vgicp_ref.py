"""The restatement of the voxelised GICP registration (tests/vgicp_ref.py) and its fixtures (tests/vgicp_fixtures.py), on the CPU:
every property the fixtures claim, the oracle (oracle/oracle_vgicp.cpp) through the judge on every fixture, and twelve deliberate mistakes
through the same judge, each rejected on a named fixture.  docs/vgicp.md has the table of bounds and measured figures."""
import numpy as np
import pytest

import vgicp_fixtures as fx
import vgicp_ref as ref
from mvil_fusion_amd import vgicp


@pytest.fixture()
def orc(oracle):
    r = vgicp.Vgicp(oracle.lib, "orc_vgicp_")
    yield r
    r.close()


# ---- fixture properties -------------------------------------------------------------------------------------------------------------------
def test_offsets_are_the_reference_sets():
    assert len(ref.offsets(1)) == 1 and len(ref.offsets(7)) == 7 and len(ref.offsets(27)) == 27
    assert ref.offsets(1) < ref.offsets(7) < ref.offsets(27)
    assert all(sum(map(abs, o)) <= 1 for o in ref.offsets(7)) and all(max(map(abs, o)) <= 1 for o in ref.offsets(27))


def test_edges_are_exact_and_need_the_divide():
    """c + j u is exact in double for every sample (so no slot is open and fused multiply-adds cannot matter), and somewhere in the set the
    reciprocal gives another voxel than the divide: the fallback of vox_coord is load-bearing on this fixture."""
    samples = inexact = differ = 0
    for axis in range(3):
        for res in fx.EDGE_RES:
            for k in fx.EDGE_K:
                n, bad = fx.exact_edge_sums(axis, res, k)
                samples += n; inexact += bad
                P, T = fx.edges(axis, res, k)
                differ += sum(ref.voxel_coord(a + T[axis, 3], res)[0] != fx.reciprocal_coord(a + T[axis, 3], res) for a in P.sx[:, axis].astype(np.float64))
                assert not any(P.correspondences(T, 1)[1])
    assert samples == 3 * 5 * 9 * 129 and inexact == 0
    assert differ >= 1
    print("edges: %d samples, %d where the reciprocal differs" % (samples, differ))


def test_offsets_fixture_counts():
    P, T, _ = fx.offsets_fixture()
    assert [ref.linearize(P, T, m, ref.F64)["n"] for m in fx.MODES] == [1, 7, 27]
    assert (ref.vr.voxel_coords(P.tx) < 0).any() and (ref.vr.voxel_coords(P.tx) > 0).any()
    assert len({c.tobytes() for c in P.tc}) == 27 and not any(P.correspondences(T, 27)[1])


@pytest.mark.parametrize("name", [c[0] for c in fx.BLOCK_CASES])
def test_blocks_have_no_open_slot(name):
    P, T, mode = fx.blocks(name)
    vox, opened, noff = P.correspondences(T, mode)
    assert not any(opened) and len(vox) == len(P.sx) * mode and any(v is not None for v in vox)
    if name == "n513":
        assert set(int(n) for n in P.map["num"]) == set(range(1, 61))


def test_two_slots_size():
    tx, tc, sx, sc, T = fx.two_slots()
    assert 2 * 128 * 512 > len(sx) * 27 == 65610 > 128 * 512           # 74 threads of k_vgicp_align take a second slot


def test_far_expects_nothing():
    P, T = fx.far()
    assert [ref.linearize(P, T, m, ref.F64)["n"] for m in fx.MODES] == [0, 0, 0]
    # what a 21-bit key does with the same coordinates
    assert ref.vr.pack_key((1 << 21) + 3, 0, 0) == ref.vr.pack_key(3, 0, 0) == ref.vr.pack_key(3 - (1 << 21), 0, 0)


def test_covariance_fixture_properties():
    x, axes = fx.lattice()
    C, _ = ref.covariances(x, fx.K, ref.F64)
    for c, a in zip(C, axes):
        assert np.abs(np.array(c) - np.diag([1e-3 if r == a else 1.0 for r in range(3)])).max() <= 8 * fx.ULP
    for swapped in (False, True):
        x = fx.tie(swapped)
        d = ref.sqdist32(x[0], x)
        assert d[1] == d[2] == 4.0 and (np.sort(d)[:19] < 4.0).all() and (d[3:] < 4.0).all()
        a, _ = ref.covariances(x, fx.K, ref.F64, points=[0]); b, _ = ref.covariances(x, fx.K, ref.F64, points=[0], larger_index_first=True)
        assert np.linalg.norm(fx._normal(a[0]) - fx._normal(b[0])) > 1e-2
    x = fx.unfused()
    A, B = 20, 19
    assert A in ref.neighbours(x, 0, fx.K) and B not in ref.neighbours(x, 0, fx.K)
    plain, _ = ref.covariances(x, fx.K, ref.F64, points=[0])
    for form in ("second", "third", "both"):
        nb = ref.neighbours(x, 0, fx.K, form)
        assert B in nb and A not in nb, form
        fused, _ = ref.covariances(x, fx.K, ref.F64, points=[0], fuse=form)
        assert np.abs(np.array(fused[0]) - np.array(plain[0])).max() > 1e-3


@pytest.mark.parametrize("kind", ["collinear", "coincident"])
def test_degenerate_invariants_hold_for_the_restatement(kind):
    C, _ = ref.covariances(fx.degenerate(kind), fx.K, ref.F64)
    fx.check_degenerate(np.array(C))


@pytest.mark.parametrize("name", list(fx.ALIGN_CASES))
def test_alignment_cases_are_decided_with_margin(name):
    m, f = fx.aligned(name, "mp"), fx.aligned(name, "f64")
    assert m["decisions"] == f["decisions"]
    assert m["n_correspondences"] >= 100 and not m["any_open"] and not f["any_open"]
    for a in (m, f):
        assert all(v >= 1e-6 for kind in ("rho", "conv", "pivot") for v in a["margins"][kind]), a["margins"]
    rejected = sum(1 for k, v in m["decisions"] if k == "reject" and v)
    if name == "poor_guess":
        assert rejected >= 1 and m["converged"] == 1
    if name == "small_budget":
        assert m["lm_failed"] == 1 and rejected >= 2
    if name in ("one_iteration", "two_iterations"):
        assert m["iterations"] == (1 if name == "one_iteration" else 2) and m["converged"] == 0
    assert all(v > 0 for v in fx.align_floors(name).values())


# ---- the oracle through the judge ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("res", fx.EDGE_RES)
def test_oracle_edges(orc, res):
    for axis in range(3):
        for k in fx.EDGE_K:
            P, T = fx.edges(axis, res, k)
            fx.load(orc, P)
            for mode in fx.MODES:
                fx.judge_linearize(orc, P, T, mode, want_H=False, tag="edges:%g/%d/%d/%d" % (res, axis, k, mode))
                if res == fx.EDGE_RES_WITH_H:
                    fx.judge_linearize(orc, P, T, mode, tag="edges:%g/%d/%d/%d/H" % (res, axis, k, mode))


def test_oracle_offsets_and_far(orc):
    P, T, _ = fx.offsets_fixture()
    fx.load(orc, P)
    for mode in fx.MODES:
        fx.judge_linearize(orc, P, T, mode, second=True, tag="offsets:%d" % mode)
    P, T = fx.far()
    fx.load(orc, P)
    for mode in fx.MODES:
        fx.judge_linearize(orc, P, T, mode, tag="far:%d" % mode)


@pytest.mark.parametrize("name", [c[0] for c in fx.BLOCK_CASES])
def test_oracle_blocks(orc, name):
    P, T, mode = fx.blocks(name)
    fx.load(orc, P)
    fx.judge_linearize(orc, P, T, mode, second=True, tag="blocks:" + name)
    fx.judge_linearize(orc, P, T, mode, want_H=False, tag="blocks:" + name + "/err")


@pytest.mark.parametrize("name", list(fx.COV_CLOUDS))
def test_oracle_covariances(orc, name):
    ok, d, fl = fx.judge_cov(orc.covariances(fx.COV_CLOUDS[name](), fx.K), name)
    print("vgicp-ref cov", name, "%.2e/%.2e" % (d, fl))
    assert ok, (d, fl)


@pytest.mark.parametrize("kind", ["collinear", "coincident"])
def test_oracle_degenerate(orc, kind):
    fx.check_degenerate(orc.covariances(fx.degenerate(kind), fx.K))


@pytest.mark.parametrize("name", list(fx.ALIGN_CASES))
def test_oracle_align(orc, name):
    P, guess, opts = fx.align_case(name)
    fx.load(orc, P)
    T, s = orc.align(guess, orc.default_options(**opts))
    ok, v = fx.judge_align(fx.summary_from(T, s), name)
    print("vgicp-ref align", name, v)
    assert ok, v


# ---- the comparison can fail: numpy mutants of the restatement through the same judge ------------------------------------------------------
def _lin_mutant(P, T, mode, **kw):
    l = ref.linearize(P, T, mode, ref.F64, **kw)
    return (l["err"], ref.to_np(l["H"]), ref.to_np(l["b"]), l["n"])


def test_mutant_reciprocal_without_fallback_fails_edges():
    failed = 0
    for axis in range(3):
        for res in fx.EDGE_RES:
            for k in fx.EDGE_K:
                P, T = fx.edges(axis, res, k)
                e, H, b, n = _lin_mutant(P, T, 1, coord=fx.reciprocal_coord, want_H=False)
                failed += not fx.judge_values((e, None, None, n), P, T, 1, want_H=False)[0]
    assert failed >= 1


def test_mutant_offsets_fail_offsets_fixture():
    P, T, _ = fx.offsets_fixture()
    assert fx.judge_values(_lin_mutant(P, T, 7), P, T, 7)[0] and fx.judge_values(_lin_mutant(P, T, 27), P, T, 27)[0]      # the unmutated route passes
    assert not fx.judge_values(_lin_mutant(P, T, 7, offs=fx.DIRECT7_MOVED), P, T, 7)[0]
    assert not fx.judge_values(_lin_mutant(P, T, 27, offs=fx.DIRECT27_WRONG_ORDER), P, T, 27)[0]


@pytest.mark.parametrize("mutant", ["w_is_num", "rcr_identity", "skew_negated"])
def test_mutant_slot_formula_fails_blocks(mutant):
    kw = dict(w_is_num=dict(w_of=lambda A, num: A.num(float(num))), rcr_identity=dict(rcr_identity=True), skew_negated=dict(skew_sign=-1))[mutant]
    P, T, mode = fx.blocks("n257")
    assert fx.judge_values(_lin_mutant(P, T, mode), P, T, mode)[0]
    ok, v = fx.judge_values(_lin_mutant(P, T, mode, **kw), P, T, mode)
    assert not ok
    if mutant == "skew_negated":                            # the error and the translation blocks do not see the sign
        assert v["err"][2] and v["H_tt"][2] and not v["H_rt"][2] and not v["b_rot"][2]


@pytest.mark.parametrize("mutant,name", [("larger_index_first", "tie"), ("larger_index_first", "tie_swapped"), ("fuse", "unfused"), ("largest", "tilted1"),
                                         ("divisor", "tilted4")])
def test_mutant_covariances_fail(mutant, name):
    xyz = fx.COV_CLOUDS[name]()
    assert fx.judge_cov(ref.covariances(xyz, fx.K, ref.F64)[0], name)[0]
    kws = dict(larger_index_first=[dict(larger_index_first=True)], fuse=[dict(fuse=f) for f in ("second", "third", "both")], largest=[dict(largest=True)],
               divisor=[dict(divisor=fx.K - 1)])[mutant]
    for kw in kws:
        assert not fx.judge_cov(ref.covariances(xyz, fx.K, ref.F64, **kw)[0], name)[0], kw


@pytest.mark.parametrize("mutant", ["lambda_without_cube", "never_reject"])
def test_mutant_optimiser_fails_poor_guess(mutant):
    """never_reject: a trial accepted on rho <= 0 as well.  Every |rho| of the fixtures is at least 1e-6, so rho = 0 does not occur and accepting
    rho <= 0 is accepting every trial."""
    P, guess, opts = fx.align_case("poor_guess")
    assert fx.judge_align(fx.summary_of(fx.aligned("poor_guess", "f64")), "poor_guess")[0]
    assert not fx.judge_align(fx.summary_of(ref.align(P, guess, opts, ref.F64, **{mutant: True})), "poor_guess")[0]
