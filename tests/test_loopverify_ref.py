"""tests/loopverify_ref.py, the NumPy restatement of vloop_score (include/villoop.h), pinned against independent implementations: the
neighbours against scipy's kd-tree, the sum against math.fsum, the boundary, tie and rounding rules on hand-made inputs.  No GPU.
The inputs built here are shared with tests/test_gpu_loopverify.py."""
import math

import numpy as np
import pytest

import loopverify_ref as ref

F32 = np.float32


def rigid(seed, max_angle=0.3, max_shift=0.5):
    """A random rigid 4 x 4 (float64; its entries are not float32 numbers)."""
    rng = np.random.default_rng(100 + seed)
    w = rng.normal(size=3); w *= rng.uniform(0.02, max_angle) / np.linalg.norm(w)
    th = np.linalg.norm(w); k = w / th
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    T = np.eye(4)
    T[:3, :3] = np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * (K @ K)
    T[:3, 3] = rng.uniform(-max_shift, max_shift, 3)
    return T


def box_pair(n_source=257, n_target=1000, seed=0):
    """(source, target): uniform random points in a 10 m box.  257 points leave a partial wave, a partial workgroup and a partial
    256-point sum block."""
    rng = np.random.default_rng(seed)
    return rng.uniform(-5.0, 5.0, (n_source, 3)).astype(F32), rng.uniform(-5.0, 5.0, (n_target, 3)).astype(F32)


def boundary_case():
    """(source, target): coordinates are small integers, so every d2 is exact: source point 0 lies on a target point, source point 1 at
    d2 = 4.0 exactly from its nearest one."""
    tgt = np.array([[0, 0, 0], [40, 0, 0], [0, 40, 0]], F32)
    src = np.array([[0, 0, 0], [2, 0, 0]], F32)
    return src, tgt


def lattice_case():
    """(source, target, expected idx): the 27 points of a 3 x 3 x 3 unit lattice, each listed twice (54 targets; point k and k + 27 are
    equal); queries at the 8 cell centres (8 lattice points at d2 = 0.75, each twice), at edge midpoints (2 at 0.25) and on lattice
    points (d2 = 0, the duplicate pair).  Everything is exact in float32; the expected index is the smallest among the nearest."""
    g = np.array([[x, y, z] for x in range(3) for y in range(3) for z in range(3)], F32)
    tgt = np.concatenate([g, g])
    src = np.array([[x + 0.5, y + 0.5, z + 0.5] for x in range(2) for y in range(2) for z in range(2)] +
                   [[0.5, 0, 0], [1, 1.5, 2], [2, 2, 0.5], [1.5, 1, 1]] + [[1, 1, 1], [2, 2, 2], [0, 0, 0]], F32)
    d = ((src[:, None, :].astype(np.float64) - tgt[None].astype(np.float64)) ** 2).sum(axis=2)          # exact in double too
    want = np.array([int(np.flatnonzero(row == row.min())[0]) for row in d], np.int32)
    return src, tgt, want


def test_neighbours_match_the_kd_tree():
    """On the same float32-transformed points: the index wherever the two best distances differ, d2 to 4 float32 ulp (the tree forms the
    distance in double, where a difference of float32 coordinates is exact; in float32 the differences, the three products and the two
    sums each round by half an ulp, which adds up to less than 4 ulp of the result)."""
    from scipy.spatial import cKDTree
    src, tgt = box_pair()
    tree = cKDTree(tgt.astype(np.float64))
    for s in range(3):
        q = ref.transform(rigid(s), src)
        d2, idx = ref.nearest(q, tgt)
        dd, ii = tree.query(q.astype(np.float64), k=2)
        clear = dd[:, 0] != dd[:, 1]
        assert clear.sum() > 250
        assert np.array_equal(idx[clear], ii[clear, 0])
        assert np.all(np.abs(d2.astype(np.float64) - dd[:, 0] ** 2) <= 4 * np.spacing(d2).astype(np.float64))
        assert idx.dtype == np.int32 and d2.dtype == F32


def test_block_sum_is_within_the_bound_of_any_summation_order():
    """|sum - fsum| <= n 2^-53 fsum holds for every order of summing n non-negative terms."""
    rng = np.random.default_rng(5)
    for n in (1, 255, 256, 257, 1000, 2400):
        d2 = (rng.uniform(0, 3, n) ** 2).astype(F32)
        for mr in (ref.DBL_MAX, 4.0):
            total, used = ref.block_total(d2, mr)
            terms = [float(v) for v in d2 if float(v) <= mr]
            exact = math.fsum(terms)
            assert used == len(terms)
            assert abs(total - exact) <= len(terms) * 2.0 ** -53 * exact
            assert ref.block_sum(d2, mr) == ((total / used if used else ref.DBL_MAX), used)


def test_block_order_is_the_declared_one():
    """Three terms whose sum depends on the order: 2^53 + 1 + 1 is 2^53 when summed left to right, 2^53 + 2 when the ones meet first.
    Point 255 closes the first block, points 256 and 257 form the second: (.. + 2^53) + (1 + 1)."""
    d2 = np.zeros(258, F32)
    d2[255] = 2.0 ** 53; d2[256] = 1.0; d2[257] = 1.0
    assert ref.block_total(d2)[0] == 2.0 ** 53 + 2.0
    d2 = np.zeros(258, F32)
    d2[0] = 2.0 ** 53; d2[1] = 1.0; d2[2] = 1.0
    assert ref.block_total(d2)[0] == 2.0 ** 53


def test_max_range_is_inclusive_and_compared_with_the_squared_distance():
    src, tgt = boundary_case()
    s, n, d2, idx = ref.score(np.eye(4), src, tgt, 4.0)
    assert d2.tolist() == [0.0, 4.0] and idx.tolist() == [0, 0]
    assert (s, n) == (2.0, 2)
    s, n, _, _ = ref.score(np.eye(4), src, tgt, np.nextafter(4.0, 0.0))
    assert (s, n) == (0.0, 1)
    s, n, _, _ = ref.score(np.eye(4), src[1:], tgt, np.nextafter(4.0, 0.0))
    assert (s, n) == (ref.DBL_MAX, 0)
    s, n, _, _ = ref.score(np.eye(4), src, tgt)
    assert (s, n) == (2.0, 2)


def test_ties_go_to_the_smaller_index():
    src, tgt, want = lattice_case()
    d2, idx = ref.nearest(src, tgt)
    assert np.array_equal(idx, want)
    assert np.all(idx < 27)
    assert d2[:8].tolist() == [0.75] * 8 and d2[8:12].tolist() == [0.25] * 4 and d2[12:].tolist() == [0.0] * 3
    d2, idx = ref.nearest(np.array([[1, 1, 1.5]], F32), np.array([[1, 1, 1], [5, 5, 5], [1, 1, 1]], F32))
    assert idx.tolist() == [0]


def test_transform_is_rounded_to_float_first():
    src, tgt = box_pair()
    T = rigid(7)
    T32 = T.astype(F32).astype(np.float64)
    assert not np.array_equal(T, T32)
    a, b = ref.score(T, src, tgt), ref.score(T32, src, tgt)
    assert a[:2] == b[:2] and np.array_equal(a[2], b[2]) and np.array_equal(a[3], b[3])
    T[3] = [3.0, -1.0, 2.0, 5.0]                                # the bottom row is not read
    assert ref.score(T, src, tgt)[:2] == a[:2]
    m = T32[0]                                                  # the unfused float32 chain, element by element
    q0 = [F32(F32(F32(F32(m[0]) * F32(v[0])) + F32(F32(m[1]) * F32(v[1]))) + F32(F32(m[2]) * F32(v[2]))) + F32(m[3]) for v in src[:16]]
    assert np.array_equal(np.array(q0, F32), ref.transform(T, src)[:16, 0])


def test_selection_rule():
    assert ref.select([0.5, 0.3, 0.3, 0.4], [1, 1, 1, 1], 1.0) == (1, F32(0.3))
    assert ref.select([0.5, 0.3], [1, 0], 1.0) == (0, F32(0.5))
    assert ref.select([0.5], [1], 0.5) == (-1, F32(0.5))
    assert ref.select([], [], 1.0) == (-1, F32(1.0))
    T = rigid(3)
    assert np.abs(ref.inverse_isometry(T) @ T - np.eye(4)).max() < 1e-15
