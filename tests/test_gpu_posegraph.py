"""The on-device pose-graph optimisation (include/vilpgo.h) against its NumPy restatement (tests/posegraph_ref.py).

Bounds and where they come from:
  * evaluation: the float64 floor of the formula -- the largest difference between the restatement in float64 and in 40-digit mpmath on the same
    inputs, per output -- times 16, the margin for the device's operation order.  The cost is one number and its float64 value met the 40-digit
    one by luck (7.3e-16 at 156); its floor is the floor of r propagated to first order, sum |r| x floor_r, and the cost is also held BIT FOR BIT to
    the header's sum of the device's own residuals.  Measured on an MI355X (floor / the device's distance from the 40-digit values):
    r 2.5e-14 / 2.3e-14, J_i 2.2e-14 / 2.2e-14, J_j 8.5e-15 / 8.5e-15, g 2.6e-12 / 2.5e-12, cost 1.8e-12 / 5.6e-14.
    The floors are set by the 3.0 rad cases (1 / sin amplifies) under whitening by up to 10.
  * one step: the componentwise backward error of the applied step in H d = -g, H and g assembled in 64-bit-mantissa arithmetic from vpgo_eval's
    output, at most 20 x that of a float64 dense LU on the same system (the bound of tests/test_gpu_step.py).  Measured: at most 3.3 x over the 54 cases.
  * converged: the gradient at the device's solution at most 10 x the one scipy reaches on the fixture, the poses within 10 x the spread of
    scipy's `lm` and `trf` solutions (posegraph_fixtures.scipy_reference, recorded by tests/test_posegraph_ref.py).  Measured (device / scipy on
    the same host): N 129 shared 1.2e-9 / 2.0e-9 and 2.3e-9 / 1.1e-8; N 129 one 3.0e-9 / 7.9e-10 and 2.4e-9 / 2.3e-9; N 65 neighbours 1.1e-9 /
    1.9e-9 and 6.6e-9 / 6.6e-9; every tenth pose 4.3e-9 / 7.9e-10 and 2.9e-9 / 2.3e-9.  The prior's information of 1e9 puts the gradient's floor
    at the spacing of the representable states: a tighter step tolerance only adds rejected attempts and leaves these figures as they are."""
import hashlib
import os
import subprocess
import sys

import numpy as np
import pytest

import posegraph_fixtures as pf
import posegraph_ref as pr
import step_ref as sr
from mvil_fusion_amd import lib, posegraph

pytestmark = pytest.mark.gpu
B = posegraph.SEGMENT
HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def so():
    return lib.load_vilsolve()


def device_graph(so, fx, batch=True, **kw):
    g = posegraph.PoseGraph(so, max_poses=kw.get("max_poses", 512), max_factors=kw.get("max_factors", 2048))
    return pf.feed(g, fx, batch)


def ref_graph(fx):
    return pf.feed(pr.Graph(), fx)


def snapshot(g):
    return hashlib.sha256(b"".join(np.ascontiguousarray(a).tobytes() for a in (g.poses(),) + tuple(np.asarray(v) for v in g.eval()))).hexdigest()


def run_digest(so):
    """what the reproducibility test compares: a graph with segments, separators, loops and position factors, built and optimised"""
    g = device_graph(so, pf.make(2 * B + 1, "shared", positions=True))
    sm = g.optimize()
    d = "%s %d %r" % (snapshot(g), sm.iterations, sm.final_cost)
    g.close()
    return d


# ---- 1. evaluation ---------------------------------------------------------------------------------------------------------------------------------
def eval_fixture():
    """Every factor kind, variances that all differ, i > j edges, and residual rotations of 0, the small-angle threshold and both of its sides, 3.0 rad."""
    rng = np.random.default_rng(5)
    N = 12
    poses = [pf.pose(0.8 * rng.standard_normal(3), 10 * rng.standard_normal(3)) for _ in range(N)]
    var = lambda n: 0.01 + rng.random(n)
    t = pr.SMALL_ANGLE
    fac = []
    for a, ang in enumerate([0.0, t * (1 - 1e-3), t, t * (1 + 1e-3), 3.0, 0.3]):
        u = rng.standard_normal(3); u /= np.linalg.norm(u)
        D = pf.pose(ang * u, 0.1 * rng.standard_normal(3))              # the residual transform
        i, j = a, (a + 5) % N
        fac.append((pr.PRIOR, i, i, poses[i] @ pr.inverse(D), var(6)))
        fac.append((pr.BETWEEN, i, j, pr.inverse(poses[i]) @ poses[j] @ pr.inverse(D), var(6)))
        hi, lo = max(i, j), min(i, j)                                   # i > j, as the reference's loop factors
        fac.append((pr.BETWEEN, hi, lo, pr.inverse(poses[hi]) @ poses[lo] @ pr.inverse(D), var(6)))
        fac.append((pr.POSITION, i, i, poses[i][:3, 3] + rng.standard_normal(3), var(3)))
    return {"N": N, "init": np.array(poses), "factors": fac, "truth": np.array(poses)}


def test_evaluation_matches_restatement_to_the_float64_floor(so):
    import mpmath
    mpmath.mp.dps = 40
    fx = eval_fixture()
    g = posegraph.PoseGraph(so, max_poses=64, max_factors=256)
    for T in fx["init"]:
        g.add_pose(T)
    for f in fx["factors"]:
        pf.add_factor(g, f)
    r, Ji, Jj, cost, grad = g.eval()
    g.close()
    ref = pr.Graph()
    for T in fx["init"]:
        ref.add_pose(T)
    for f in fx["factors"]:
        pf.add_factor(ref, f)
    r64, Ji64, Jj64 = ref.linearize()
    c64, g64 = ref.cost_of(r64), ref.gradient(r64, Ji64, Jj64)
    to_mp = lambda a: np.array([mpmath.mpf(float(v)) for v in np.asarray(a, np.float64).ravel()], dtype=object).reshape(np.shape(a))
    rm, Jim, Jjm = [], [], []
    for kind, i, j, Z, var in fx["factors"]:
        a, b_, c_ = pr.factor_eval(kind, to_mp(fx["init"][i]), to_mp(fx["init"][j]), to_mp(Z), to_mp(var), m=mpmath)
        rm.append(a); Jim.append(b_); Jjm.append(c_)
    rm, Jim, Jjm = np.array(rm), np.array(Jim), np.array(Jjm)
    cm = sum(v * v for v in rm.ravel()) / 2
    gm = np.array([[mpmath.mpf(0)] * 6] * fx["N"], dtype=object)
    for f, (kind, i, j, _, _) in enumerate(fx["factors"]):
        gm[i] = gm[i] + Jim[f].T @ rm[f]
        if kind == pr.BETWEEN:
            gm[j] = gm[j] + Jjm[f].T @ rm[f]
    dist = lambda a, m: float(max(abs(mpmath.mpf(float(x)) - y) for x, y in zip(np.asarray(a, np.float64).ravel(), np.asarray(m, dtype=object).ravel())))
    for name, dev, f64, mp in (("r", r, r64, rm), ("J_i", Ji, Ji64, Jim), ("J_j", Jj, Jj64, Jjm), ("g", grad, g64, gm), ("cost", [cost], [c64], [cm])):
        floor, d = dist(f64, mp), dist(dev, mp)
        if name == "r":
            floor_r = floor
        if name == "cost":
            # one number can agree with the 40-digit value by luck (the float64 sum did, to 7.3e-16 at a value of 156, under half a unit in its
            # last place): the cost's floor is the floor of r carried through d cost = sum r dr to first order, sum |r| x floor_r
            floor = float(np.abs(r64).sum()) * floor_r
        print("evaluation %-4s float64 floor %.3e device distance %.3e" % (name, floor, d))
        assert floor > 0 and d <= 16 * floor, (name, floor, d)
    assert cost == ref.cost_of(r), "the cost is not the header's sum of the device's own residuals"


# ---- 2. one step -----------------------------------------------------------------------------------------------------------------------------------
def assemble(fx_factors, r, Ji, Jj, N, dtype):
    H, g = np.zeros((6 * N, 6 * N), dtype), np.zeros(6 * N, dtype)
    for f, (kind, i, j, _, _) in enumerate(fx_factors):
        a, rr = Ji[f].astype(dtype), r[f].astype(dtype)
        si = slice(6 * i, 6 * i + 6)
        H[si, si] += a.T @ a; g[si] += a.T @ rr
        if kind == pr.BETWEEN:
            b_ = Jj[f].astype(dtype); sj = slice(6 * j, 6 * j + 6)
            H[sj, sj] += b_.T @ b_; g[sj] += b_.T @ rr
            H[si, sj] += a.T @ b_; H[sj, si] += b_.T @ a
    return H, g


@pytest.mark.parametrize("layout", pf.LAYOUTS)
@pytest.mark.parametrize("N", pf.SIZES)
def test_gauss_newton_step_backward_error(so, N, layout):
    fx = pf.make(N, layout)
    g = device_graph(so, fx)
    r, Ji, Jj, _, _ = g.eval()
    before = g.poses()
    sm = g.optimize(max_iterations=1, initial_lambda=0.0)
    after = g.poses()
    step = g.step().ravel()
    nsep = g.size()[2]
    g.close()
    assert (sm.iterations, sm.accepted) == (1, 1) and sm.final_cost < sm.initial_cost and sm.reduced_size == 6 * nsep, (sm.iterations, sm.accepted, sm.initial_cost, sm.final_cost)
    # The chart-local difference of the states is the step -- to the rounding of the state it was added to: a float64 LU's own step, put through
    # retract and local on the CPU, comes back with a backward error of 1e-12 .. 1e-11 on these fixtures (20 m coordinates, steps of 1e-6 .. 1),
    # a hundred times the bound below.  So the solve is judged on the step as the device holds it (vpgo_get_step), and the states are held to
    # that step within their own rounding: a few units in the last place of the rotation entries and of the largest coordinate.
    moved = np.concatenate([pr.local(a, b_) for a, b_ in zip(before, after)])
    slack = 8 * np.finfo(np.float64).eps * (1.0 + float(np.abs(before[:, :3, 3]).max()))
    assert np.abs(moved - step).max() <= slack, (N, layout, float(np.abs(moved - step).max()), slack)
    fac = pf.ordered_factors(fx)
    H, grad = assemble(fac, r, Ji, Jj, N, sr.LD)
    om = sr.omega(H, -grad, step)
    x64 = np.linalg.solve(H.astype(np.float64), -grad.astype(np.float64))
    om64 = sr.omega(H, -grad, x64)
    print("N %d %s: %d loops, %d separators, %d segments, omega %.3e omega64 %.3e ratio %.2f" % (N, layout, len(pf.loops(N, layout)), nsep, sm.n_segments, om, om64, om / om64))
    assert om <= 20 * om64, (N, layout, om, om64)


# ---- 3. converged ----------------------------------------------------------------------------------------------------------------------------------
CONVERGED = [(2 * B + 1, "shared"), (2 * B + 1, "one"), (B + 1, "neighbours")]
# scipy runs to the rounding floor of the gradient; the default cost_tolerance stops two or three iterations before that (the damping slows the
# weakly held global translation), so the comparison runs until the step itself is below 1e-11
TIGHT = dict(cost_tolerance=0.0, step_tolerance=1e-11)


def check_converged(fx, poses, tag):
    ref = pf.scipy_reference(fx)
    rg = pr.Graph()
    rg.poses = [T.copy() for T in poses]
    rg.factors = pf.ordered_factors(fx)
    r, Ji, Jj = rg.linearize()
    gn = float(np.abs(rg.gradient(r, Ji, Jj)).max())
    dist = float(max(np.abs(pr.local(a, b_)).max() for a, b_ in zip(ref["poses"], poses)))
    print("%s: |J^T r|_inf %.3e (scipy %.3e), distance to scipy %.3e (lm/trf spread %.3e)" % (tag, gn, ref["grad"], dist, ref["spread"]))
    assert gn <= 10 * ref["grad"], (tag, gn, ref["grad"])
    assert dist <= 10 * ref["spread"], (tag, dist, ref["spread"])
    return ref


@pytest.mark.parametrize("N,layout", CONVERGED)
def test_converged_from_drifted_odometry(so, N, layout):
    fx = pf.make(N, layout, positions=True)
    g = device_graph(so, fx)
    sm = g.optimize(**TIGHT)
    poses = g.poses()
    g.close()
    print("N %d %s: %d iterations (%d accepted), cost %.6g -> %.6g, termination %d, lambda %.3g" % (N, layout, sm.iterations, sm.accepted, sm.initial_cost, sm.final_cost, sm.termination, sm.final_lambda))
    assert sm.termination == posegraph.TERM_STEP and 2 <= sm.iterations < 20 and sm.accepted >= 2 and sm.final_cost < sm.initial_cost
    ref = check_converged(fx, poses, "N %d %s" % (N, layout))
    end = lambda P: float(np.linalg.norm(np.asarray(P)[-1][:3, 3] - fx["truth"][-1][:3, 3]))
    e0, e_dev, e_ref = end(fx["init"]), end(poses), end(ref["poses"])
    print("end-of-loop position error: drifted %.4f m, device %.4f m, restatement %.4f m" % (e0, e_dev, e_ref))
    assert abs(e_dev - e_ref) <= 10 * ref["spread"] and e_ref < e0


# ---- 4. incremental equals batch -----------------------------------------------------------------------------------------------------------------------
def test_incremental_build_gives_the_same_bits_as_batch(so):
    fx = pf.make(2 * B + 1, "shared", positions=True)
    a, b_ = device_graph(so, fx, batch=True), device_graph(so, fx, batch=False)
    assert snapshot(a) == snapshot(b_)
    sa, sb = a.optimize(), b_.optimize()
    assert (sa.iterations, sa.final_cost) == (sb.iterations, sb.final_cost) and snapshot(a) == snapshot(b_)
    a.close(); b_.close()


def test_optimising_every_tenth_pose_ends_at_the_same_minimum(so):
    fx = pf.make(2 * B + 1, "one", positions=True)
    g = posegraph.PoseGraph(so, max_poses=512, max_factors=2048)
    n = 0
    for kind, v in pf.events(fx):
        if kind == "pose":
            if n and n % 10 == 0:
                g.optimize()
            # a new pose starts from the optimised previous pose and the odometry measurement, as the reference's initial value does
            T = v if n == 0 else g.poses(n - 1, 1)[0] @ [f for f in fx["factors"] if f[0] == pr.BETWEEN and f[1] == n - 1 and f[2] == n][0][3]
            g.add_pose(T); n += 1
        else:
            pf.add_factor(g, v)
    sm = g.optimize(**TIGHT)
    poses = g.poses()
    g.close()
    assert sm.termination == posegraph.TERM_STEP and sm.iterations < 20
    check_converged(fx, poses, "every tenth pose")


def test_relative_is_the_alignment_guess(so):
    """vpgo_relative(i, j) = T_j^-1 T_i (pose2.inv() * pose1, :370), and vpgo_get_poses returns what was added"""
    fx = pf.make(9, "one")
    g = device_graph(so, fx)
    P = g.poses()
    assert np.array_equal(P, fx["init"]) and np.array_equal(g.poses(3, 2), fx["init"][3:5])
    want = pr.inverse(P[2]) @ P[8]
    got = g.relative(8, 2)
    g.close()
    assert np.abs(got - want).max() <= 4 * np.finfo(np.float64).eps * (1.0 + np.abs(P[:, :3, 3]).max())      # three products and a sum per entry


# ---- 5. bit reproducibility ----------------------------------------------------------------------------------------------------------------------------
def test_bit_reproducible_across_runs_and_processes(so):
    a, b_ = run_digest(so), run_digest(so)
    assert a == b_
    out = subprocess.run([sys.executable, os.path.join(HERE, "posegraph_child.py")], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    child = [l for l in out.stdout.splitlines() if l.startswith("digest ")]
    assert child == ["digest " + a], (child, a)


# ---- 6. error paths ------------------------------------------------------------------------------------------------------------------------------------
def test_errors_leave_the_graph_unchanged(so):
    fx = pf.make(B + 1, "one", positions=True)
    g = posegraph.PoseGraph(so, max_poses=B + 1, max_factors=len(fx["factors"]) + 1)
    pf.feed(g, fx)
    want, size = snapshot(g), g.size()
    I, v6, nan = np.eye(4), np.full(6, 0.05), float("nan")
    bad = np.eye(4); bad[1, 3] = float("inf")
    cases = [("i == j", lambda: g.add_between(3, 3, I, v6), -1), ("key out of range", lambda: g.add_between(0, B + 1, I, v6), -1),
             ("negative key", lambda: g.add_prior(-1, I, v6), -1), ("position key", lambda: g.add_position(B + 1, np.zeros(3), np.ones(3)), -1),
             ("zero variance", lambda: g.add_between(0, 5, I, [0.05, 0.05, 0.0, 0.05, 0.05, 0.05]), -1),
             ("negative variance", lambda: g.add_position(2, np.zeros(3), [1.0, -1.0, 1.0]), -1), ("nan variance", lambda: g.add_prior(2, I, [nan] * 6), -1),
             ("inf variance", lambda: g.add_prior(2, I, [float("inf")] * 6), -1),
             ("non-finite measurement", lambda: g.add_between(0, 5, bad, v6), -3), ("non-finite position", lambda: g.add_position(1, [0.0, nan, 0.0], np.ones(3)), -3),
             ("non-finite pose", lambda: g.add_pose(bad), -3), ("pose capacity", lambda: g.add_pose(I), posegraph.ERR_CAPACITY)]
    for tag, call, status in cases:
        with pytest.raises(posegraph.PoseGraphError) as e:
            call()
        assert e.value.status == status, (tag, e.value.status)
        assert g.size() == size and snapshot(g) == want, tag
    g.add_between(0, 2, fx["factors"][1][3], v6)                        # the last free factor slot
    want, size = snapshot(g), g.size()
    with pytest.raises(posegraph.PoseGraphError) as e:
        g.add_between(0, 3, I, v6)
    assert e.value.status == posegraph.ERR_CAPACITY and g.size() == size and snapshot(g) == want
    g.close()


def test_separator_capacity_is_refused_at_add_between(so):
    N = 4 * B + 3
    fx = pf.make(N, "full")
    g = device_graph(so, fx)
    assert g.size()[2] == posegraph.MAX_SEPARATORS
    want, size = snapshot(g), g.size()
    free = [k for k in range(2, N) if (k, k - 2) not in pf.loops(N, "full")]
    with pytest.raises(posegraph.PoseGraphError) as e:
        g.add_between(free[-1], free[-1] - 2, np.eye(4), np.full(6, 0.05))
    assert e.value.status == posegraph.ERR_CAPACITY and g.size() == size and snapshot(g) == want
    g.close()


# ---- 7. end to end with vloop_verify --------------------------------------------------------------------------------------------------------------------
def test_verified_loop_goes_into_the_graph(so):
    """The delta and fitness of vloop_verify on the tiny clouds of test_gpu_loopverify.py go straight into vpgo_add_between (the reference's
    BetweenFactor(current, history, delta, Variances(fitness)), :387); the optimised graph equals the restatement fed the same numbers."""
    from mvil_fusion_amd import loopverify, vgicp
    tx, _, sx, _, _ = vgicp.make_pair(0, rings=8, az=300)
    guess = np.eye(4); guess[:3, 3] = [0.1, -0.04, 0.01]
    reg = vgicp.Vgicp(so); lv = loopverify.LoopVerify(so, max_points=4096)
    best, _ = lv.verify(reg, sx, [(tx, guess)])
    lv.close(); reg.close()
    assert best.index == 0
    delta, fitness = loopverify.mat(best.delta), float(best.fitness)
    N = 12
    fx = pf.make(N, "none", seed=3)
    fx["factors"].append((pr.BETWEEN, N - 1, 0, delta, np.full(6, fitness)))
    g = device_graph(so, fx)
    sm = g.optimize(**TIGHT)
    poses = g.poses()
    g.close()
    print("loop factor from vloop_verify (fitness %.4g): %d iterations, cost %.9g -> %.9g" % (fitness, sm.iterations, sm.initial_cost, sm.final_cost))
    assert sm.termination == posegraph.TERM_STEP and sm.iterations < 20 and sm.final_cost < sm.initial_cost
    rg = ref_graph(fx)
    it, c0, c1, term = rg.optimize(**TIGHT)
    dist = float(max(np.abs(pr.local(a, b_)).max() for a, b_ in zip(rg.poses, poses)))
    print("restatement's own minimiser: %d iterations, termination %d, cost %.9g, distance %.3e" % (it, term, c1, dist))
    # the same factors and numbers: the initial cost to its own rounding (13 factors x 6 terms); both minimisers stop at a step below 1e-11, and
    # with a contraction no slower than 0.999 per iteration (measured: 1/3, the damping's decay) each is then within 1e-11 / (1 - 0.999) = 1e-8
    # of the minimum; the cost is flat there (second order in that distance)
    assert term == 1 and abs(sm.initial_cost - c0) <= 1e-12 * c0 and dist <= 1e-8 and abs(sm.final_cost - c1) <= 1e-10 * c1
