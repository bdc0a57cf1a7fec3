"""vmap_associate / vmap_align (csrc/vilmap.hip, vil_knn.hpp, vil_pose1.hpp) against the 50-digit restatement of tests/mapreg_ref.py on the fixtures of
tests/mapreg_fixtures.py -- nothing of oracle/oracle_map.cpp judges here, except the DECISION on the two rule-dependent (rank-deficient) plane fits.

  D1  accepted scan points, in scan order: identical to the restatement's on every query it decides (gate margin above tau); none of the designed cases and
      at most 1 % of the random fixture may be undecided.
  D2  a, b (up to the swap the sign of u allows), n, d: within 16 x the float64 floor of the class -- the largest distance between the restatement's float64
      route (numpy eigh / lstsq) and its 50-digit values over the fixtures that share a scale (the room, the hand-placed cases, the cases 500 m out).
  D3  on the rounding-sensitive queries and the lattices the neighbours are those of the UNFUSED float32 sum, as include/vilmap.h promises.
  D4  vmap_align with max_iterations = 0, one-launch path and window-solver path: n_edge, n_plane of the restatement and its 50-digit initial cost
      (factors_ref.lidar_residual, Huber 0.1, identity extrinsic) within 16 x the cost's float64 floor sum |r| x floor_r (tests/test_gpu_posegraph.py).
  E   the first trust-region step of the solve (Jacobi scaling, Cholesky with rsqrt_nr pivots, dogleg; csrc/vil_pose1.hpp): vmap_align capped at one
      iteration, at the default radius (Gauss-Newton branch) and at initial_radius = 1e-3 (Cauchy branch), one-launch and window-solver path, against the
      extended-precision route of tests/step_ref.py applied twice on the restatement's factors (mapreg_ref.two_rounds / check_two_rounds: only the pose after
      round two comes back through the C ABI, so it is read as round two's step from the reference's intermediate pose and the rounding of the two stored
      poses, step_ref.read_noise, is carried in the bound).

Measured on an MI355X (float64 floor / the device's largest distance from the 50-digit values):
  the room + the sensitive queries   a, b 1.8e-15 / 4.4e-16    n 2.0e-14 / 1.2e-14    d 8.3e-14 / 3.9e-14
  the hand-placed cases              a, b 2.2e-16 / 1.1e-16    n 4.1e-14 / 3.8e-14    d 1.5e-13 / 1.2e-13      (n, d: the plane 1e-3 m from the origin, |n| = 1e3)
  the cases 500 m out                a, b 2.8e-14 / 0          n 1.7e-13 / 9.6e-14    d 1.8e-12 / 1.1e-12
  initial cost 0.870100232027418 (77 edges, 207 planes): floor 3.6e-13, both solve paths 5.5e-15 away.
  Every floor is the measured distance between numpy's route and the 50-digit values, except a, b of the cases 500 m out: there eigh lands on the rounded
  50-digit values (measured 0) and the floor is the half unit in the last place that mapreg_ref.floors never goes below (2.8e-14 at 400 m).
  E, relative to the largest scaled component of round two's step (0.040 at the default radius, 6.5e-4 at 1e-3):
    Gauss-Newton   forward error one-launch 2.6e-13, window 1.7e-13 (float64 route 2.6e-13; read noise 3.7e-12)
                   backward error omega one-launch 1.5e-13, window 8.7e-14 (float64 LU on the same system 1.8e-13; read noise carried 7.1e-12)
    Cauchy         forward error 1.9e-11 on both paths = the float64 route's (all three store the same pose; read noise 2.2e-10)
  What E resolves is set by the stored pose's rounding (2^-52 of a 2 m translation against a step of 1e-3 .. 4e-2), not by the margin of 20: through this
  ABI a step wrong by 1e-8 of itself is caught (tests/test_mapreg_ref.py shows it), one wrong by 1e-12 is not.
No class needs the margin of 16: rsqrt_nr / rcp_nr and the division-free Jacobi rotation sit inside the floor of numpy's eigh / lstsq.  The two rank-deficient
plane fits are rejected by device and oracle alike.
D3's outcome: the promise did NOT hold.  With the searches instantiated with sqdist_nofma (STRICT = false) the 32 sensitive queries came back with another set
of five neighbours (a, b up to 0.38 m from the unfused answer): the back end fuses that sum.  csrc/vilmap.hip now searches with STRICT = true and every case
above passes.  k_map_search by vmap_profile_read at bench.py's sizes (60000 + 8000 map, 6000 + 800 scan points, 300 launches per process, the two libraries
alternating, three processes each): 18.6 / 18.4 / 18.4 us before, 19.6 / 18.2 / 18.9 us after -- inside the spread between processes.
"""
import numpy as np
import pytest

import factors_ref as fr
import mapreg_fixtures as mf
import mapreg_ref as mr
from mvil_fusion_amd import abi, lib, mapreg

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def tables(oracle):
    """every fixture through vmap_associate and orc_vmap_associate, once.  A context keeps its grids' cell sizes from one map to the next, so every fixture
    gets a fresh one: the lattices are then searched at cell size 1, where their exact distances of 1.0f ARE ring bounds, and the crowded map at 0.125
    (mapreg_fixtures.cell_size; tests/test_mapreg_ref.py checks both)."""
    vil, out = lib.load_vilsolve(), {}
    for name in mf.names():
        fx = mf.get(name)
        g = mapreg.MapReg(vil, "vmap_"); o = mapreg.MapReg(oracle.lib, "orc_vmap_")
        for r in (g, o):
            r.set_map(fx.cmap, fx.smap)
        out[name] = (g.associate(fx.sc, fx.ss, fx.q, fx.t), o.associate(fx.sc, fx.ss, fx.q, fx.t))
        g.close(); o.close()
    return out


@pytest.mark.parametrize("group", mf.GROUP_NAMES)
def test_accepted_set_and_values(tables, group):
    """D1 + D2"""
    names = mf.group(group)
    floor = mr.floors(names)
    measured = mr.floors(names, clamp=False)
    assert all(v > 0 for v in floor.values()), floor
    assert all(measured[c] > 0 for c in mr.CLASSES if (group, c) != ("far", "ab")), measured      # the float64 route really differs from the 50-digit one
    worst, n_open, n_rule, failed = dict.fromkeys(mr.CLASSES, 0.0), 0, 0, []
    for name in names:
        (edge, plane), (oe, op) = tables[name]
        problems, dist, rule, opened = mr.judge(mr.cached(name), edge, plane, floor=floor)
        rule_o = mr.judge(mr.cached(name), oe, op)[2]
        assert opened == 0 or name == "random", name                                  # no designed case hides inside tau
        n_open += opened; n_rule += len(rule)
        if rule != rule_o:
            problems.append(("rule-dependent decision differs from the oracle's", rule, rule_o))
        worst = {c: max(worst[c], dist[c]) for c in mr.CLASSES}
        if problems:
            failed.append((name, problems[:4]))
    for c in mr.CLASSES:
        print("%-8s %-2s float64 floor %.3e device distance %.3e (%.2f floors)" % (group, c, floor[c], worst[c], worst[c] / floor[c]))
    assert n_open <= 4 and n_rule == (2 if group == "designed" else 0)               # 1 % of the random fixture's 400 queries
    assert not failed, failed


@pytest.mark.parametrize("name", ["sensitive", "lattice_int_corner", "lattice_quarter_corner", "lattice_half_surf", "lattice_int_surf_ring_bound"])
def test_neighbours_are_those_of_the_unfused_float_sum(tables, name):
    """D3.  On the sensitive fixture some fused form of the sum hands the fit another five points: the emitted line then moves by centimetres, so the class
    floor separates the two outcomes by ten orders of magnitude.  The lattices have exact sums: every form agrees, only the search's own logic can differ."""
    assoc = mr.cached(name)
    floor = mr.floors(mf.group("random" if name == "sensitive" else "designed"))
    problems, dist, _, opened = mr.judge(assoc, *tables[name][0], floor=floor)
    if name == "sensitive":
        fx = mf.get(name)
        other = 0
        for rec in assoc.corner:
            for v, (vn, vd, vg) in rec.fused.items():
                if set(vn.tolist()) != set(rec.nn.tolist()) and mr.status(rec) == "accept":
                    alt = mr.corner_fit(fx.cmap[vn, :3])
                    other += mr._dist("ab", alt.value, rec) > 1e6 * floor["ab"]
                    break
        assert other >= 24, other                                                      # the fused outcome would have been told apart
    assert opened == 0 and not problems, problems[:6]


def _cost(S, edge, plane, pose7):
    """(0.5 sum rho(|r|^2), residuals) with HuberLoss(0.1) (ceres: rho(s) = s for s <= a^2, 2 a sqrt(s) - a^2 above), identity extrinsic"""
    P, Q = fr.pose_tangent(S, pose7)
    a, total, rs = S.c(0.1), S.zero, []
    for kind, rows in ((0, edge), (2, plane)):
        for row in rows:
            r, _ = fr.lidar_residual(S, kind, list(row), [0.0, 0.0, 0.0, 1.0], [0.0, 0.0, 0.0], P, Q)
            s = sum((x * x for x in r), S.zero)
            total = total + S.half * (s if s <= a * a else S.c(2.0) * a * S.sqrt(s) - a * a)
            rs += list(r)
    return total, rs


@pytest.mark.parametrize("path", ["one_launch", "window"])
def test_both_solve_paths_see_the_restatements_tables(hip, path):
    """D4"""
    fx, assoc = mf.get("random"), mr.cached("random")
    assert not any(mr.status(r) in ("open", "rule") for r in assoc.corner + assoc.surf)
    pose7 = [float(v) for v in np.concatenate([fx.t, fx.q])]
    c_mp, r_mp = _cost(fr.MP, mr.tables(assoc.corner), mr.tables(assoc.surf), pose7)
    c64, r64 = _cost(fr.F64, mr.tables(assoc.corner, use64=True), mr.tables(assoc.surf, use64=True), pose7)
    floor_r = max(abs(float(fr.MP.c(a) - b)) for a, b in zip(r64, r_mp))
    floor = float(np.abs(r64).sum()) * floor_r
    g = mapreg.MapReg(lib.load_vilsolve(), "vmap_")
    if path == "window":
        assert g.lib.vmap_set_fused_max(g.ctx, 0) == 0
    g.set_map(fx.cmap, fx.smap)
    q, t, s = g.align(hip.ctx, fx.sc, fx.ss, fx.q, fx.t, abi.default_options(max_iterations=0))
    g.close()
    d = abs(float(fr.MP.c(s.initial_cost) - c_mp))
    print("%s: n_edge %d n_plane %d initial cost %.17g (50 digits %.17g, float64 route %.17g) floor %.3e device distance %.3e" % (
        path, s.n_edge, s.n_plane, s.initial_cost, float(c_mp), c64, floor, d))
    assert (s.rounds, s.n_edge, s.n_plane, s.iterations) == (2, len(mr.tables(assoc.corner)), len(mr.tables(assoc.surf)), 0)
    assert np.array_equal(q, fx.q) and np.array_equal(t, fx.t)
    assert floor > 0 and d <= 16 * floor, (floor, d)


@pytest.mark.parametrize("path", ["one_launch", "window"])
@pytest.mark.parametrize("radius", [1e4, 1e-3])
def test_first_step_of_the_solve(hip, path, radius):
    """E.  vmap_align capped at one iteration: each of its two rounds is one dogleg step from a fresh trust-region state, and only the pose after round two
    comes back through the C ABI.  So the reference route is applied twice (mapreg_ref.two_rounds) and the returned pose is read as round two's step from the
    50-digit route's intermediate pose, with step_ref.read_step / read_noise; mapreg_ref.check_two_rounds states the bounds and why the rounding of the stored
    poses enters them.  The tolerances are zeroed so that no round ends before its step is judged."""
    ref = mr.two_rounds(radius)
    fx = mf.get("random")
    g = mapreg.MapReg(lib.load_vilsolve(), "vmap_")
    if path == "window":
        assert g.lib.vmap_set_fused_max(g.ctx, 0) == 0
    g.set_map(fx.cmap, fx.smap)
    q, t, s = g.align(hip.ctx, fx.sc, fx.ss, fx.q, fx.t, abi.default_options(max_iterations=1, initial_radius=radius, function_tolerance=0.0, parameter_tolerance=0.0))
    g.close()
    assert (s.rounds, s.iterations, s.n_edge, s.n_plane) == (2, 1, ref.rounds[1].n_edge, ref.rounds[1].n_plane) and s.final_cost < s.initial_cost
    fig = mr.check_two_rounds(ref, np.concatenate([t, q]), path)
    assert (fig.branch == "gauss_newton") == (radius == 1e4)
