"""The scan-to-map association's restatement (tests/mapreg_ref.py) and its fixtures (tests/mapreg_fixtures.py), on the CPU:

  * every property the fixtures are built for holds at 50 digits (gate margins above the decision floor tau, exact ties, exact distances, the crowded cell,
    at least 32 rounding-sensitive queries);
  * oracle/oracle_map.cpp's orc_vmap_associate -- until now compared with nothing but itself -- accepts the same scan points in scan order wherever the
    restatement decides, and emits a, b, n, d within 16 x the float64 floor of tests/test_gpu_map_floor.py's bound;
  * the comparison can fail: five deliberate mistakes in the restatement's expectations are each caught on every fixture they change.
"""
import numpy as np
import pytest

import mapreg_fixtures as mf
import mapreg_ref as mr
from mvil_fusion_amd import mapreg

F32 = np.float32


def recs(name):
    a = mr.cached(name)
    return a.corner + a.surf


def run(reg, fx):
    reg.set_map(fx.cmap, fx.smap)
    return reg.associate(fx.sc, fx.ss, fx.q, fx.t)


@pytest.fixture(scope="module")
def oracle_tables(oracle):
    r = mapreg.MapReg(oracle.lib, "orc_vmap_")
    out = {n: run(r, mf.get(n)) for n in mf.names()}
    r.close()
    return out


# ---- fixture properties -----------------------------------------------------------------------------------------------------------------------------------
def test_designed_cases_are_decided_with_margin():
    """B1 - B4: no query within tau of a gate, none with an open transform; the cases built for one outcome have it; rule-dependent exactly where meant"""
    for b in mf.DESIGNED:
        for name in mf.names(b):
            want = mf.get(name).tags.get("expect")
            for rec in recs(name):
                st = mr.status(rec)
                assert st != "open", (name, rec.index)
                assert (st == "rule") == (want == "rule"), (name, st)
                if want in ("accept", "reject"):
                    assert st == want, (name, rec.index, st)
                if rec.fit is not None and not rec.fit.rule_dependent:
                    assert abs(rec.fit.margin) > rec.fit.tau > 0


def test_random_fixture_is_decided_but_for_one_percent():
    rs = recs("random")
    assert len(rs) == 400 and sum(mr.status(r) == "open" for r in rs) <= len(rs) // 100
    assert sum(mr.status(r) == "accept" for r in rs if not r.surf) > 40 and sum(mr.status(r) == "accept" for r in rs if r.surf) > 150
    assert len(mf.get("random").cmap) == 600 and len(mf.get("random").smap) == 2000


def test_gate_edges_sit_where_they_are_meant_to():
    for name in mf.names("B1"):
        rel = mf.get(name).tags.get("gate_rel")
        if rel is not None:
            (rec,) = recs(name)
            ratio = float(rec.fit.lam[2] / rec.fit.lam[1])
            assert abs(ratio / 3.0 - 1.0 - rel) < 0.3 * abs(rel) and rec.fit.ok == (rel > 0), (name, ratio)
    for name in mf.names("B2"):
        off = mf.get(name).tags.get("gate_abs")
        if off is not None:
            (rec,) = recs(name)
            assert abs((0.2 - rec.fit.margin) - (0.2 + off)) < 0.3 * abs(off) and rec.fit.ok == (off < 0), (name, rec.fit.margin)
    (rec,) = recs("plane_near_origin_1e-3")
    assert 0.9e-3 < rec.fit.value[3] < 1.1e-3
    assert 499.0 < recs("plane_far_500m")[0].fit.value[3] < 501.0 and np.linalg.norm(recs("corner_far_500m")[0].fit.centre) > 499.0
    assert 5e-5 < np.ptp(mf.get("corner_spread_1e-4").cmap[:, 0]) < 1e-3


def test_degenerate_corner_cases():
    (rec,) = recs("corner_identical")
    assert not rec.fit.A.any() and not rec.fit.ok                                    # 0 > 0
    for name in ("corner_collinear", "corner_axis_line"):
        (rec,) = recs(name)
        u, want = np.array([float(x) for x in rec.fit.u]), mf.get(name).tags["direction"]
        assert float(rec.fit.lam[1]) < 1e-40 * float(rec.fit.lam[2]) and rec.fit.ok and min(np.abs(u - want).max(), np.abs(u + want).max()) < 1e-15
    A = recs("corner_axis_line")[0].fit.A
    assert not (A - np.diag(np.diag(A))).any()                                       # Jacobi's off == 0 exit
    A = recs("corner_one_zero_pair")[0].fit.A
    assert np.array_equal(A * 256, [[160, 0, 32], [0, 4, -4], [32, -4, 12]])         # exactly one zero off-diagonal pair, and it is the first one visited
    seen = set()
    for name in mf.names("B1"):
        pq = mf.get(name).tags.get("pq")
        if pq:
            A = recs(name)[0].fit.A
            p, q = pq
            d, apq = A[q, q] - A[p, p], A[p, q]
            assert d != 0 and apq != 0 and not A[3 - p - q].any()                    # the line lies in the axis plane: the third row of the scatter is zero
            seen.add((pq, d > 0, apq > 0))
    assert len(seen) == 12                                                           # three planes x the four sign combinations of the rotation's `pos`


def test_intensity_ties_and_picks():
    for name in mf.names("B3"):
        fx = mf.get(name)
        (rec,) = recs(name)
        diff = np.abs(fx.smap[rec.nn, 3] - fx.ss[0, 3])
        kept = sorted(diff)[4]
        assert np.sum(diff == kept) >= 2 and np.sum(diff <= kept) > 5, name          # an exact tie decides the fifth place
        assert np.sum(diff == kept) >= fx.tags["ties"]
        if fx.tags.get("not_nearest"):
            assert set(rec.picks) != set(rec.nn[:5].tolist())
    for name in mf.names("B2"):
        (rec,) = recs(name)
        assert set(rec.picks) != set(rec.nn[:5].tolist()), name                      # the picks are the five with the query's intensity, not the five nearest


def test_search_fixture_properties():
    one, below = F32(1.0), np.nextafter(F32(1.0), F32(0.0))
    for name in mf.names("B4"):
        fx = mf.get(name)
        rs = recs(name)
        if "d5_is_one" in fx.tags:
            assert sum(r.d5 == one for r in rs) == fx.tags["d5_is_one"], name
            assert all(not r.gate for r in rs if r.d5 == one)
        if "d10_is_one" in fx.tags:
            assert sum(r.d[-1] == one and r.d5 < one and r.gate for r in rs if r.surf) == fx.tags["d10_is_one"]       # the tenth distance IS the ring bound
        if "tie_queries" in fx.tags:
            for i in fx.tags["tie_queries"]:
                d6 = mr.knn(rs[i].s, fx.cmap, 6)[1]
                assert d6[4] == d6[5] and rs[i].gate                                   # the fifth place is decided by the index
    assert recs("gate_d5_exactly_one")[0].d5 == one and not recs("gate_d5_exactly_one")[0].gate
    assert recs("gate_d5_below_one")[0].d5 == below and recs("gate_d5_below_one")[0].gate
    assert any(np.any(mf.get(n).sc[:, :3] < 0) or np.any(mf.get(n).ss[:, :3] < 0) for n in mf.names("B4"))
    for name in ("lattice_int_corner", "lattice_quarter_corner", "lattice_half_surf", "lattice_int_surf_ring_bound"):
        fx = mf.get(name)
        for M in (fx.cmap, fx.smap, fx.sc, fx.ss):
            assert np.array_equal(M[:, :3] * 8, np.round(M[:, :3] * 8))                # eighth-lattice coordinates: every product and sum is exact in float32
        assert not any(r.list_sensitive for r in recs(name))
        for M in (fx.cmap, fx.smap):                                                   # a fresh context keeps cell size 1: 1.0f IS the first ring's bound there
            assert len(M) == 0 or mf.cell_size(M) == 1.0, name
    assert (len(mf.get("map_4_and_9").cmap), len(mf.get("map_4_and_9").smap), len(mf.get("map_5_and_10").cmap), len(mf.get("map_5_and_10").smap)) == (4, 9, 5, 10)
    assert recs("map_4_and_9") == [] and len(recs("map_5_and_10")) == 2
    fx = mf.get("crowded_cell")
    for M in (fx.cmap, fx.smap):
        assert mf.cell_size(M) == mf.CELL_MIN                                         # a fresh context: 1 -> sqrt(6 / 600) = 0.1, clamped to 0.125
        for h in (1.0, 0.5, 0.25, mf.CELL_MIN):
            assert len(M) > 512 and len(np.unique(np.floor(M[:, :3] / F32(h)), axis=0)) == 1   # one cell at both sizes of that build (and the powers of two between)


def test_rounding_sensitive_queries():
    rs = recs("sensitive")
    assert len(rs) >= 32 and all(r.sensitive and r.gate and not r.surf for r in rs)
    for r in rs:                                                                       # some fused sum hands the fit another set of five
        assert any(set(v[0].tolist()) != set(r.nn.tolist()) for v in r.fused.values())
    assert sum(mr.status(r) == "accept" for r in rs) >= 24                             # and most of them show it in an emitted factor


def test_rule_dependent_flag_is_the_rank_test():
    for name in ("plane_rule_collinear", "plane_rule_pairs"):
        (rec,) = recs(name)
        assert rec.fit.rule_dependent and rec.fit.sv[2] <= mr.RANK_TOL * rec.fit.sv[0] and np.linalg.matrix_rank(rec.fit.P) == 2
    assert not any(r.fit.rule_dependent for r in recs("random") if r.fit is not None)


# ---- the oracle against the restatement ----------------------------------------------------------------------------------------------------------------------
def test_oracle_matches_restatement(oracle_tables):
    worst = dict.fromkeys(mr.CLASSES, 0.0)
    for group in mf.GROUP_NAMES:
        names = mf.group(group)
        floor = mr.floors(names)
        measured = mr.floors(names, clamp=False)                                      # before the half-ulp clamp: the two routes really differ
        assert all(v > 0 for v in floor.values()), (group, floor)
        assert all(measured[c] > 0 for c in mr.CLASSES if (group, c) != ("far", "ab")), (group, measured)       # far a, b: eigh lands on the rounded 50-digit values
        for name in names:
            problems, dist, rule, n_open = mr.judge(mr.cached(name), *oracle_tables[name], floor=floor)
            assert not problems, (name, problems[:5])
            worst = {c: max(worst[c], dist[c] / floor[c]) for c in mr.CLASSES}
        print("group %-8s floors %s before the half-ulp clamp %s" % (group, {c: "%.2e" % v for c, v in floor.items()}, {c: "%.2e" % v for c, v in measured.items()}))
    print("oracle's largest distance in floors:", {c: "%.2f" % v for c, v in worst.items()})


# ---- sharpness ---------------------------------------------------------------------------------------------------------------------------------------------
MUST_APPLY = {"col1": ["random", "corner_collinear", "corner_gate_+1e-06", "crowded_cell"], "lam0": ["corner_gate_-1e-06", "corner_gate_-0.001"],
              "norerank": ["random", "rerank_all_equal", "rerank_tie_off_plane_first", "plane_gate_+1e-06"], "ge": ["random", "gate_d5_below_one", "map_5_and_10"],
              "le": ["gate_d5_exactly_one"]}


@pytest.mark.parametrize("defect", sorted(MUST_APPLY))
def test_a_wrong_expectation_is_caught(oracle_tables, defect):
    """The oracle's tables judged against a deliberately wrong restatement: every fixture whose expectation the mistake changes must report a problem."""
    applied = []
    for group in mf.GROUP_NAMES:
        names = mf.group(group)
        floor = mr.floors(names)
        for name in names:
            fx, good = mf.get(name), mr.cached(name)
            bad = mr.associate(fx.cmap, fx.smap, fx.sc, fx.ss, fx.q, fx.t, defect=defect, with_fused=False)
            changed = False
            for g, b in zip(good.corner + good.surf, bad.corner + bad.surf):
                sg, sb = mr.status(g), mr.status(b)
                changed |= sg != sb and "open" not in (sg, sb) and "rule" not in (sg, sb)
                if sg == sb == "accept":
                    changed |= any(mr._dist(c, b.fit.value, g) > 1e-6 for c in (("n", "d") if g.surf else ("ab",)))
            if changed:
                applied.append(name)
                problems = mr.judge(bad, *oracle_tables[name], floor=floor)[0]
                assert problems, (defect, name)
    assert set(MUST_APPLY[defect]) <= set(applied), (defect, sorted(set(MUST_APPLY[defect]) - set(applied)))


# ---- the first step of the solve: the oracle's, and the check's own sharpness ---------------------------------------------------------------------------------
STEP_OPTS = dict(max_iterations=1, function_tolerance=0.0, parameter_tolerance=0.0)       # one dogleg step per round, never ended early by a tolerance
STEP_RADII = (1e4, 1e-3)                                                                  # the Gauss-Newton branch (the default radius) / a trust region the step must be cut to


@pytest.mark.parametrize("radius", STEP_RADII)
def test_oracle_first_step(oracle, radius):
    """orc_vmap_align held to the two-round reference route of mapreg_ref.two_rounds, as tests/test_gpu_map_floor.py holds vmap_align; and a step that is wrong
    in one component by one part in 10^8 of itself fails the same check."""
    from mvil_fusion_amd import abi
    ref = mr.two_rounds(radius)
    fx = mf.get("random")
    for rnd in ref.rounds:
        assert rnd.branch == rnd.branch64 == ("gauss_newton" if radius == 1e4 else rnd.branch) and (radius == 1e4 or rnd.branch != "gauss_newton")
        assert not rnd.undecided and rnd.n_edge > 40 and rnd.n_plane > 150
    r = mapreg.MapReg(oracle.lib, "orc_vmap_")
    r.set_map(fx.cmap, fx.smap)
    q, t, s = r.align(None, fx.sc, fx.ss, fx.q, fx.t, abi.default_options(initial_radius=radius, **STEP_OPTS))
    r.close()
    assert (s.rounds, s.iterations, s.n_edge, s.n_plane) == (2, 1, ref.rounds[1].n_edge, ref.rounds[1].n_plane) and s.final_cost < s.initial_cost
    mr.check_two_rounds(ref, np.concatenate([t, q]), "oracle")
    wrong = np.concatenate([t, q])
    wrong[1] += 1e-8 * abs(float(ref.rounds[1].ld.s[1] * ref.rounds[1].y[1]))
    with pytest.raises(AssertionError):
        mr.check_two_rounds(ref, wrong, "oracle, t_y step off by 1e-8 of itself")
