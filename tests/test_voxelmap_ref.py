"""The restatement of the target voxel map (tests/voxelmap_ref.py) against hand-computed maps, and the self-checks of the fixtures that the GPU
tests (tests/test_gpu_voxelmap.py) compare both builders with.  No GPU."""
import numpy as np

import voxelmap_ref as ref

F = np.float32


def test_pack_key_and_hash_key_by_hand():
    assert ref.pack_key(0, 0, 0) == 0 and ref.pack_key(1, 0, 0) == 1 << 42 and ref.pack_key(0, 1, 0) == 1 << 21 and ref.pack_key(0, 0, 1) == 1
    assert ref.pack_key(-1, 0, 2) == (0x1FFFFF << 42) | 2
    assert ref.pack_key(-1, -1, -1) == (1 << 63) - 1                     # 63 bits: never negative as a signed 64-bit integer
    assert ref.hash_key(0) == 0 and ref.hash_key(1) == 0x9E3779B9 and ref.hash_key(2) == 0x3C6EF372
    assert ref.hash_key(1 << 42) == ((0x9E3779B97F4A7C15 << 42) & 0xFFFFFFFFFFFFFFFF) >> 32


def test_two_voxels_by_hand():
    # x / 0.5 - 0.5: 0.375 -> 0.25, 0.875 -> 1.25, 0.625 -> 0.75: voxels 0, 1, 0; every number below is exact in binary
    xyz = np.array([[0.375, 0.375, 0.375], [0.875, 0.375, 0.375], [0.625, 0.375, 0.375]], F)
    cov = np.array([np.arange(1, 10), 10 * np.arange(1, 10), 100 * np.arange(1, 10)], np.float64)
    m = ref.build(xyz, cov, 0.5)
    assert m["keys"].tolist() == [0, 1 << 42] and m["num"].tolist() == [2, 1]
    assert m["mean"].tolist() == [[0.5, 0.375, 0.375], [0.875, 0.375, 0.375]]
    assert m["cov"].tolist() == [[50.5 * q for q in range(1, 10)], [10.0 * q for q in range(1, 10)]]
    assert m["wsq"].tolist() == [2.0 ** 0.5, 1.0]
    assert m["keys"].dtype == np.int64 and m["num"].dtype == np.int32 and m["mean"].dtype == m["cov"].dtype == m["wsq"].dtype == np.float64


def test_three_voxels_by_hand_numbered_by_first_point():
    # the negative voxel comes first, the voxel of points 1 and 3 second, a single point last
    xyz = np.array([[-0.125, 0.375, 1.375], [0.375, 0.375, 0.375], [0.875, 0.375, 0.375], [0.625, 0.125 + 0.25, 0.5]], F)
    cov = np.array([np.full(9, 1.0), np.full(9, 2.0), np.full(9, 8.0), np.full(9, 4.0)])
    m = ref.build(xyz, cov, 0.5)
    assert m["keys"].tolist() == [(0x1FFFFF << 42) | 2, 0, 1 << 42] and m["num"].tolist() == [1, 2, 1]
    assert m["mean"].tolist() == [[-0.125, 0.375, 1.375], [0.5, 0.375, 0.4375], [0.875, 0.375, 0.375]]
    assert m["cov"].tolist() == [[1.0] * 9, [3.0] * 9, [8.0] * 9]
    # another resolution: at 1.0 every point has a voxel of its own
    assert ref.voxel_coords(xyz, 1.0).tolist() == [[-1, -1, 0], [-1, -1, -1], [0, -1, -1], [0, -1, 0]]


def test_key_boundaries():
    """A coordinate of exactly k * 0.5 + 0.25 belongs to voxel k, its lower float neighbour to k - 1, its upper one to k."""
    pts = ref.boundary_cloud(0.5)
    assert pts.shape == (63, 3) and pts.dtype == F
    vc = ref.voxel_coords(pts, 0.5)
    row = 0
    for axis in range(3):
        for k in range(-3, 4):
            assert float(pts[row + 1, axis]) == k * 0.5 + 0.25
            assert pts[row, axis] < pts[row + 1, axis] < pts[row + 2, axis]
            assert [vc[row + j, axis] for j in range(3)] == [k - 1, k, k], (axis, k)
            others = [a for a in range(3) if a != axis]
            assert (vc[row:row + 3, others] == -1).all()                 # 0.1 / 0.5 - 0.5 = -0.3
            row += 3
    m = ref.build(pts, ref.plain_cov(len(pts)), 0.5)
    assert int(m["num"].sum()) == 63 and len(m["keys"]) == len(set(m["keys"].tolist()))


def test_signed_zeros():
    """The sums start from 0.0: 0.0 + (-0.0) is +0.0, so a voxel of nothing but -0.0 has the mean +0.0."""
    pts = ref.zero_cloud()
    assert pts.shape == (8, 3) and np.signbit(pts[0]).all() and not np.signbit(pts[7]).any()
    cov = np.zeros((8, 9)); cov[:, ::2] = -0.0
    m = ref.build(pts, cov, 0.5)
    assert m["keys"].tolist() == [ref.pack_key(-1, -1, -1)] and m["num"].tolist() == [8]
    assert not np.signbit(m["mean"]).any() and not np.signbit(m["cov"]).any() and (m["mean"] == 0).all()
    one = ref.build(pts[:1], cov[:1], 0.5)
    assert np.signbit(pts[:1]).all() and not np.signbit(one["mean"]).any() and not np.signbit(one["cov"]).any()
    neg = one["mean"].copy(); neg[:] = -0.0
    assert not ref.same_map(one, dict(one, mean=neg))                    # the byte comparison tells the zeros apart


def test_order_fixture_exposes_the_order_of_the_sums():
    """Means of float coordinates are exact in double at these counts, whatever the order; the covariance sums are not.  Reversing
    one voxel's additions must change at least one bit, or a GPU test on this fixture could pass by accident."""
    for n_total, n_a in ((600, 300), (257, 129), (1025, 513)):
        xyz, cov, which = ref.order_fixture(n_total)
        assert len(xyz) == n_total and int((which == 0).sum()) == n_a
        assert which[:8].tolist() == [0, 1, 0, 2, 0, 1, 0, 2]
        m = ref.build(xyz, cov)
        assert m["num"].tolist() == [n_a, int((which == 1).sum()), int((which == 2).sum())]
        assert ref.order_matters(xyz, cov, which, 0), n_total
        mag = np.abs(cov)
        assert mag.min() >= 1e-3 and mag.max() < 2e3 and (cov < 0).any() and (cov > 0).any()
    xyz, cov, which = ref.order_fixture(600)
    assert np.nonzero(which == 0)[0][128] == 256                         # the run of voxel A crosses the edge of the first 256 points


def test_collision_fixture_collides():
    coords = ref.collision_coords()
    assert coords.shape == (48, 3) and np.abs(coords).max() <= 40
    keys = [ref.pack_key(*c) for c in coords]
    assert len(set(keys)) == 48
    assert len({ref.hash_key(k) & 4095 for k in keys}) == 1              # one start slot in any table of up to 4096 slots
    assert len({ref.hash_key(k) for k in keys}) > 1
    for per_key in (1, 2):
        xyz, cov, cc = ref.collision_fixture(per_key)
        assert len(xyz) == 48 * per_key
        assert (ref.voxel_coords(xyz) == cc).all()
        m = ref.build(xyz, cov)
        assert m["keys"].tolist() == keys and (m["num"] == per_key).all()


def test_population_fixtures():
    xyz, cov = ref.population_fixture("one_voxel")
    m = ref.build(xyz, cov)
    assert m["num"].tolist() == [2049]
    xyz, cov = ref.population_fixture("all_own")
    m = ref.build(xyz, cov)
    assert len(xyz) == 3000 and (m["num"] == 1).all() and len(m["num"]) == 3000
    assert np.array_equal(m["mean"], xyz.astype(np.float64)) and np.array_equal(m["cov"], cov)       # x / 1 is x
    xyz, cov = ref.population_fixture("counts_1_to_60")
    m = ref.build(xyz, cov)
    assert sorted(m["num"].tolist()) == list(range(1, 61)) and len(xyz) == 1830
    for k in range(1, 8):
        assert m["wsq"][m["num"] == k * k].tolist() == [float(k)]                                    # exact roots exactly


def test_restatement_matches_a_vectorised_count():
    """Independent of the loop: the number of points per key and the order of the keys' first points."""
    rng = np.random.default_rng(3)
    xyz = rng.uniform(-4, 4, (5000, 3)).astype(F)
    m = ref.build(xyz, ref.plain_cov(5000))
    pk = ref.point_keys(xyz)
    uniq, first, counts = np.unique(pk, return_index=True, return_counts=True)
    by_first = np.argsort(first)
    assert m["keys"].tolist() == uniq[by_first].tolist() and m["num"].tolist() == counts[by_first].tolist()
    v = 7
    members = np.nonzero(pk == m["keys"][v])[0]
    assert np.allclose(m["mean"][v], xyz[members].astype(np.float64).mean(axis=0), rtol=1e-15, atol=0)
