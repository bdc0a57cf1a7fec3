"""GPU parity of the alignment fitness score and the loop-closure verification (include/villoop.h) with their NumPy restatement
(tests/loopverify_ref.py), through the C-ABI, bit for bit: per-point distances and indices, counts, scores, and the decision."""
import numpy as np
import pytest

import loopverify_ref as ref
from mvil_fusion_amd import lib, loopverify as lv, vgicp
from test_loopverify_ref import boundary_case, box_pair, lattice_case, rigid

pytestmark = pytest.mark.gpu

F32 = np.float32
GRID, BRUTE = 0, 1 << 30                                   # vloop_set_grid's min_points: every target / no target goes through the grid


def same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


@pytest.fixture(scope="module")
def so():
    return lib.load_vilsolve()


@pytest.fixture()
def ctx(so):
    c = lv.LoopVerify(so, max_points=4096)
    yield c
    c.close()


@pytest.fixture(scope="module")
def scans():
    """The project's synthetic scan pair at 8 x 300 = 2400 points per scan: (target, source, T_true)."""
    tx, _, sx, _, T_true = vgicp.make_pair(0, rings=8, az=300)
    return tx, sx, T_true


def check(c, Ts, src, tgt, max_range=ref.DBL_MAX, what=""):
    """One batched vloop_score against the restatement, everything compared bit for bit.  Returns the device's (scores, n_used, d2, idx)."""
    Ts = np.asarray(Ts, np.float64).reshape(-1, 4, 4)
    s, n, d2, idx = c.score(Ts, max_range, debug=True)
    for k, T in enumerate(Ts):
        es, en, ed2, eidx = ref.score(T, src, tgt, max_range)
        assert same(d2[k], ed2), (what, k, np.flatnonzero(d2[k] != ed2)[:8])
        assert same(idx[k], eidx), (what, k, np.flatnonzero(idx[k] != eidx)[:8])
        assert n[k] == en and same(np.float64(s[k]), np.float64(es)), (what, k, s[k], es, n[k], en)
    return s, n, d2, idx


@pytest.mark.parametrize("path", [GRID, BRUTE])
def test_exactness(ctx, path):
    src, tgt = box_pair(257, 1000)
    ctx.set_grid(path, 1.0)
    ctx.set_source(src); ctx.set_target(tgt)
    check(ctx, [rigid(s) for s in range(3)], src, tgt)
    check(ctx, [rigid(1)], src, tgt, 0.25, "max_range 0.25")


@pytest.mark.parametrize("cell", [1.0, 0.125])
def test_both_search_paths_return_the_same_bits(ctx, cell):
    src, tgt = box_pair(257, 300, seed=3)
    Ts = [rigid(s) for s in range(3)]
    ctx.set_source(src)
    ctx.set_grid(GRID, cell); ctx.set_target(tgt)
    a = check(ctx, Ts, src, tgt, what="grid %g" % cell)
    ctx.set_grid(BRUTE, cell)                              # after set_target: takes effect at the next score
    b = ctx.score(np.array(Ts), debug=True)
    ctx.set_grid(GRID, cell)                               # and back: the grid is rebuilt inside the submission
    c = ctx.score(np.array(Ts), debug=True)
    for x, y, z in zip(a, b, c):
        assert same(x, y) and same(x, z)


def test_far_queries_take_the_exhaustive_fallback(ctx, scans):
    src, tgt = box_pair(257, 1000, seed=4)
    far = src.copy(); far[:, 0] += F32(50.0)
    mix = src.copy(); mix[::2, 0] += F32(50.0)
    ctx.set_grid(GRID, 1.0); ctx.set_target(tgt)
    for cloud, what in ((far, "far"), (mix, "half far")):
        ctx.set_source(cloud)
        s, _, d2, _ = check(ctx, [np.eye(4), rigid(2)], cloud, tgt, what=what)
        assert (d2[0] > 36.0).sum() >= (257 if what == "far" else 128)          # beyond KNN_RMAX = 6 cells of 1 m
    tx, sx, _ = scans
    shift = np.eye(4); shift[0, 3] = 50.0
    ctx.set_source(sx)
    for path in (GRID, BRUTE):
        ctx.set_grid(path, 0.5); ctx.set_target(tx)
        s, _, _, _ = check(ctx, [shift], sx, tx, what="scan pair shifted 50 m")
        assert 1500.0 < s[0] < 1700.0                      # about 1593 on the CPU


@pytest.mark.parametrize("path", [GRID, BRUTE])
def test_ties_and_degenerate_sizes(ctx, path):
    ctx.set_grid(path, 1.0)
    src, tgt, want = lattice_case()
    ctx.set_source(src); ctx.set_target(tgt)
    _, _, d2, idx = check(ctx, [np.eye(4)], src, tgt, what="lattice")
    assert np.array_equal(idx[0], want) and idx[0].max() < 27
    one = np.array([[0.25, -1.5, 2.0]], F32)
    ctx.set_target(one)                                     # n_target == 1
    _, _, _, idx = check(ctx, [np.eye(4), rigid(0)], src, one, what="one target point")
    assert not idx.any()
    src2, tgt2 = box_pair(257, 300, seed=6)
    ctx.set_source(src2[:1]); ctx.set_target(tgt2)          # n_source == 1
    check(ctx, [rigid(1)], src2[:1], tgt2, what="one source point")
    bs, bt = boundary_case()
    ctx.set_source(bs); ctx.set_target(bt)
    s, n, d2, _ = check(ctx, [np.eye(4)], bs, bt, 4.0, "d2 == max_range")
    assert (s[0], n[0], d2[0].tolist()) == (2.0, 2, [0.0, 4.0])
    s, n, _, _ = check(ctx, [np.eye(4)], bs, bt, np.nextafter(4.0, 0.0), "just below")
    assert (s[0], n[0]) == (0.0, 1)
    ctx.set_source(bs[1:])
    s, n, _, _ = check(ctx, [np.eye(4)], bs[1:], bt, np.nextafter(4.0, 0.0), "nothing used")
    assert (s[0], n[0]) == (ref.DBL_MAX, 0)


def test_batch_repeats_and_a_new_target(so, ctx):
    src, tgt = box_pair(257, 1000, seed=8)
    _, tgt_b = box_pair(257, 700, seed=9)
    Ts = np.array([rigid(s) for s in range(3)])
    ctx.set_grid(GRID, 1.0)
    ctx.set_source(src); ctx.set_target(tgt)
    batch = check(ctx, Ts, src, tgt)
    for k in range(3):                                      # n_T = 3 equals three single calls
        s, n, d2, idx = ctx.score(Ts[k], debug=True)
        assert same(np.float64(s), np.float64(batch[0][k])) and n == batch[1][k] and same(d2, batch[2][k]) and same(idx, batch[3][k])
    again = ctx.score(Ts, debug=True)
    other = lv.LoopVerify(so, max_points=1000)              # a second context, sized to the clouds exactly
    other.set_grid(GRID, 1.0); other.set_source(src); other.set_target(tgt)
    second = other.score(Ts, debug=True)
    other.close()
    for x, y, z in zip(batch, again, second):
        assert same(x, y) and same(x, z)
    ctx.set_target(tgt_b)                                   # a new cloud invalidates the old search structure
    swapped = check(ctx, Ts, src, tgt_b, what="after the swap")
    assert not same(swapped[2], batch[2])
    ctx.set_target(tgt)
    back = ctx.score(Ts, debug=True)
    for x, y in zip(batch, back):
        assert same(x, y)


def test_chain_with_vgicp(so, ctx, scans):
    """Align from the identity, then score: the alignment lowers the score, and the score at its result is the restatement's."""
    tx, sx, _ = scans
    reg = vgicp.Vgicp(so)
    reg.set_target(tx, None, 0.5); reg.set_source(sx)
    T, summ = reg.align(np.eye(4))
    reg.close()
    assert summ.converged == 1
    ctx.set_source(sx); ctx.set_target(tx)
    s, _, _, _ = check(ctx, [T, np.eye(4)], sx, tx)
    print("score at the alignment %.6f, at the identity %.6f" % (s[0], s[1]))
    assert s[0] < s[1]


def test_verify(so, ctx, scans):
    tx, sx, _ = scans
    rng = np.random.default_rng(11)
    ball = rng.normal(size=(500, 3)); ball *= (2.0 * rng.uniform(0, 1, (500, 1)) ** (1 / 3)) / np.linalg.norm(ball, axis=1, keepdims=True)
    # make_pair's scan at pose A does not depend on dt (it would be a third copy of tx): the fourth candidate is the scan taken at the
    # doubled offset, a different cloud of the same room
    tx2 = vgicp.make_pair(0, rings=8, az=300, dt=(0.24, -0.10, 0.04))[2]
    guess = np.eye(4); guess[:3, 3] = [0.1, -0.04, 0.01]                       # entries that are not float32 numbers
    cands = [(ball.astype(F32), np.eye(4)), (tx, guess), (tx, guess), (tx2, guess)]
    opts = lv.default_options(so, max_tolerable_fitness=1.0)
    reg = vgicp.Vgicp(so)
    best, per = ctx.verify(reg, sx, cands, opts)
    # the same steps composed in Python on contexts of their own
    reg2 = vgicp.Vgicp(so); lv2 = lv.LoopVerify(so, max_points=4096)
    reg2.set_source(sx); lv2.set_source(sx)
    fit, conv, Ts, used = [], [], [], []
    for xyz, g in cands:
        reg2.set_target(xyz, None, opts.resolution); lv2.set_target(xyz)
        T, sm = reg2.align(np.asarray(g, np.float64).astype(F32).astype(np.float64), opts.reg)
        T = T.astype(F32).astype(np.float64)
        f, n = F32(lv.FLT_MAX), 0
        if sm.converged:
            s, n = lv2.score(T)
            f = F32(s)
            es, en, _, _ = ref.score(T, sx, xyz)
            assert same(np.float64(s), np.float64(es)) and n == en
        fit.append(f); conv.append(sm.converged); Ts.append(T); used.append(int(n))
        r = per[len(fit) - 1]
        assert (r.converged, r.iterations, r.n_used) == (sm.converged, sm.iterations, n)
        assert same(F32(r.fitness), f) and same(lv.mat(r.T), T)
    reg2.close(); lv2.close()
    print("fitness", fit, "converged", conv)
    want, run = ref.select(fit, conv, 1.0)
    assert conv[1] == 1 and fit[1] < 1.0
    assert best.index == want and want in (1, 3) and same(F32(best.fitness), run) and best.n_used == used[want]
    assert same(fit[1], fit[2]) and best.index != 2                              # of the two identical candidates the earlier one wins
    T, delta = lv.mat(best.T), lv.mat(best.delta)
    assert same(T, Ts[want])
    assert np.abs(delta - ref.inverse_isometry(T)).max() <= 1e-15              # two inverses of a matrix with condition number 1: a few roundings apart
    assert np.abs(delta @ T - np.eye(4)).max() <= 1e-12
    # max_tolerable_fitness exactly the winning fitness: strict <, nobody wins
    none, _ = ctx.verify(reg, sx, cands, lv.default_options(so, max_tolerable_fitness=float(run)))
    assert none.index == -1 and same(F32(none.fitness), run) and same(lv.mat(none.T), np.eye(4))
    # n_cand == 1: performSC_ICP's acceptance
    one, per1 = ctx.verify(reg, sx, cands[1:2], opts)
    assert one.index == 0 and same(F32(one.fitness), fit[1]) and same(F32(per1[0].fitness), fit[1])
    one, _ = ctx.verify(reg, sx, cands[1:2], lv.default_options(so, max_tolerable_fitness=float(fit[1])))
    assert one.index == -1
    empty, pe = ctx.verify(reg, sx, [], opts)
    assert empty.index == -1 and pe == []
    reg.close()


def test_error_paths(so, ctx):
    src, tgt = box_pair(257, 300)
    E = lv.LoopVerifyError

    def status(fn):
        with pytest.raises(E) as e:
            fn()
        return e.value.status

    assert status(lambda: ctx.score(np.eye(4))) == -1                            # no resident pair
    ctx.set_source(src)
    assert status(lambda: ctx.score(np.eye(4))) == -1                            # no target yet
    ctx.set_target(tgt)
    good = ctx.score(np.eye(4), debug=True)
    big = np.zeros((4097, 3), F32)
    assert status(lambda: ctx.set_target(big)) == -1 and status(lambda: ctx.set_source(big)) == -1
    assert status(lambda: ctx.set_target(np.zeros((0, 3), F32))) == -1
    bad = tgt.copy(); bad[17, 1] = np.nan
    assert status(lambda: ctx.set_target(bad)) == -3
    bad[17, 1] = np.inf
    assert status(lambda: ctx.set_source(bad)) == -3
    assert status(lambda: ctx.score(np.zeros((0, 4, 4)))) == -1
    assert status(lambda: ctx.score(np.tile(np.eye(4), (lv.MAX_BATCH + 1, 1, 1)))) == -1
    T = np.eye(4); T[1, 3] = np.inf
    assert status(lambda: ctx.score(T)) == -3
    assert status(lambda: ctx.score(np.eye(4), max_range=float("nan"))) == -1
    assert status(lambda: ctx.set_grid(0, 0.0)) == -1 and status(lambda: ctx.set_grid(-1, 1.0)) == -1
    again = ctx.score(np.eye(4), debug=True)                                     # a refused call leaves the resident pair as it was
    for x, y in zip(good, again):
        assert same(np.asarray(x), np.asarray(y))
    assert len(ctx.score(np.tile(np.eye(4), (lv.MAX_BATCH, 1, 1)))[0]) == lv.MAX_BATCH
    reg = vgicp.Vgicp(so)
    assert status(lambda: ctx.verify(reg, src, [(big, np.eye(4))])) == -1
    assert status(lambda: ctx.verify(reg, big, [(tgt, np.eye(4))])) == -1
    assert status(lambda: ctx.verify(reg, src, [(tgt, T)])) == -3
    assert status(lambda: ctx.verify(reg, src, [(tgt, np.eye(4))], lv.default_options(so, resolution=0.0))) == -1
    reg.close()
