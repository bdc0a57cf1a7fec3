"""tests/depthreg_ref.py (the float32 restatement of get_depth that the GPU is compared with) pinned on hand-built inputs whose answers
are known without it.  Both matrices are the identity here: the cloud is given in the view frame (x forward, y left, z up)."""
import numpy as np

import depthreg_ref as ref

EYE = np.eye(4, dtype=np.float32)[:3]


def at(row, col, rng, inten=1.0):
    """A point at the centre of range-image bin (row, col), `rng` metres away."""
    e, c = np.deg2rad(np.asarray(row, np.float64) * 0.5 - 90.0), np.deg2rad(np.asarray(col, np.float64) * 0.5)
    r = np.broadcast_to(np.asarray(rng, np.float64), np.broadcast(e, c).shape)
    return np.stack([r * np.cos(e) * np.sin(c), r * np.cos(e) * np.cos(c), r * np.sin(e), np.broadcast_to(inten, r.shape)], axis=-1).astype(np.float32).reshape(-1, 4)


def patch(rng, r0=180, c0=180):
    """3 x 3 bins around (r0, c0); rng: scalar or 9 ranges in row-major order."""
    rr, cc = np.meshgrid(np.arange(r0 - 1, r0 + 2), np.arange(c0 - 1, c0 + 2), indexing="ij")
    return at(rr.ravel(), cc.ravel(), rng)


FILL = at(np.full(6, 100), np.arange(100, 106), 9.0)           # six bins far from every feature used here: the sphere reaches 10 points
CENTRE = np.array([[0.0, 0.0, 1.0]], np.float32)               # the image centre: sphere point (1, 0, 0) = bin (180, 180)


def test_closest_point_wins_its_bin_and_the_lower_index_wins_a_tie():
    d = at(180, 180, 1.0)[0, :3]
    cloud = np.array([[*(5 * d), 1], [*(4 * d), 2], [*(6 * d), 3]], np.float32)
    o = ref.register(cloud, EYE, EYE, CENTRE)
    assert (o.n_cloud, o.n_in_view, o.n_sphere) == (3, 3, 1)
    assert o.sphere_src.tolist() == [1] and o.sphere_rc.tolist() == [[180, 180]] and abs(o.sphere[0, 3] - 4.0) < 1e-6
    assert np.allclose(o.sphere[0, :3], d, atol=1e-6)
    tie = np.array([[*(6 * d), 1], [*(4 * d), 2], [*(4 * d), 3], [*(4 * d), 4]], np.float32)
    assert ref.register(tie, EYE, EYE, CENTRE).sphere_src.tolist() == [1]
    assert ref.register(tie[::-1], EYE, EYE, CENTRE).sphere_src.tolist() == [0]


def test_centre_of_a_patch_at_range_5():
    o = ref.register(np.concatenate([FILL, patch(5.0)]), EYE, EYE, CENTRE)
    assert o.n_sphere == 15 and o.n_with_depth == 1
    assert o.nn3[0, 0] == 6 + 4 and set(o.nn3[0].tolist()) <= set(range(6, 15))      # the centre bin first: emission puts FILL's row 100 first
    assert abs(o.depth[0] - 5.0) < 1e-5                                                # p.x = 1


def test_spread_of_2_5_metres_gives_no_depth():
    rng = np.full(9, 7.5); rng[4] = 5.0
    o = ref.register(np.concatenate([FILL, patch(rng)]), EYE, EYE, CENTRE)
    assert o.nn3[0, 0] == 10 and o.depth[0] == -1 and o.n_with_depth == 0


def test_plane_at_2_9_metres_gives_no_depth():
    o = ref.register(np.concatenate([FILL, patch(2.9)]), EYE, EYE, CENTRE)
    assert o.nn3[0, 0] == 10 and o.depth[0] == -1                                       # accepted, then depth <= 3
    assert ref.register(np.concatenate([FILL, patch(3.1)]), EYE, EYE, CENTRE).depth[0] > 3.0


def test_nine_sphere_points_give_no_depth():
    o = ref.register(patch(5.0), EYE, EYE, CENTRE)
    assert o.n_sphere == 9 and o.depth.tolist() == [-1.0] and o.nn3.tolist() == [[-1, -1, -1]]
    assert ref.register(np.concatenate([FILL[:1], patch(5.0)]), EYE, EYE, CENTRE).depth[0] > 3.0       # ten do


def test_point_straight_below_lands_in_row_0():
    """x = 0, y = 0, z < 0: step 3 gives row 0 (and column 0).  Step 2 runs first, though: y / x is NaN and passes, z / x is -inf and
    |z / x| > 10 skips the point, in the reference as here -- |z / x| <= 10 keeps every surviving point between rows 11 and 349."""
    row, col = ref.bins(np.float32([0.0]), np.float32([0.0]), np.float32([-5.0]))
    assert (int(row[0]), int(col[0])) == (0, 0)
    o = ref.register(np.array([[0.0, 0.0, -5.0, 1.0]], np.float32), EYE, EYE, CENTRE)
    assert (o.n_in_view, o.n_sphere) == (0, 0)
    steep = ref.register(at([11, 349], [180, 180], 5.0), EYE, EYE, CENTRE)               # 84.5 degrees: tan = 10.4 > 10; 84 degrees passes
    assert steep.n_in_view == 0
    assert ref.register(at([12, 348], [180, 180], 5.0), EYE, EYE, CENTRE).sphere_rc[:, 0].tolist() == [12, 348]


def test_roundf_is_c_roundf():
    v = np.float32([0.5, 1.5, 2.5, -0.5, -2.5, 0.49999997, 359.5, 2.4999998])
    assert ref.roundf(v).tolist() == [1.0, 2.0, 3.0, -1.0, -3.0, 0.0, 360.0, 2.0]


def test_emission_is_row_major():
    cloud = at([201, 200, 201, 200], [151, 151, 150, 150], [5.0, 6.0, 7.0, 8.0])
    o = ref.register(cloud, EYE, EYE, CENTRE)
    assert o.sphere_rc.tolist() == [[200, 150], [200, 151], [201, 150], [201, 151]]
    assert o.sphere_src.tolist() == [3, 1, 2, 0] and np.allclose(o.sphere[:, 3], [8.0, 6.0, 7.0, 5.0], atol=1e-5)


def test_view_filter_and_dropped_points():
    cloud = np.array([[-1.0, 0.0, 0.0, 1], [1.0, 10.5, 0.0, 1], [1.0, 0.0, -10.5, 1], [1.0, 9.5, 0.0, 1], [np.nan, 0, 0, 1], [np.inf, 1.0, 0, 1], [0.0, 0.0, 0.0, 1]], np.float32)
    o = ref.register(cloud, EYE, EYE, CENTRE)
    assert o.n_cloud == 7 and o.sphere_src.tolist() == [3]


def test_fronto_parallel_wall():
    """A wall x = D seen head-on: a feature theta off the axis gets a depth within cos(theta) / cos(theta + 2.5 deg) - 1 of D (its three
    neighbours are less than 2.5 degrees away on a plane): 1.8 % at 20 degrees; 2.5 % leaves the float slack."""
    D = 8.0
    a = np.deg2rad(np.arange(-28.0, 28.01, 0.3))
    el, az = np.meshgrid(a, a, indexing="ij")
    d = np.stack([np.cos(el) * np.cos(az), np.cos(el) * np.sin(az), np.sin(el)], axis=-1).reshape(-1, 3)
    cloud = np.concatenate([d * (D / d[:, :1]), np.ones((len(d), 1))], axis=1).astype(np.float32)
    rng = np.random.default_rng(3)
    th, ph = np.deg2rad(rng.uniform(0.0, 20.0, 40)), rng.uniform(0, 2 * np.pi, 40)
    feat = np.stack([np.tan(th) * np.cos(ph), np.tan(th) * np.sin(ph), np.ones(40)], axis=1).astype(np.float32)
    o = ref.register(cloud, EYE, EYE, feat)
    assert o.n_with_depth == 40
    bound = np.cos(np.deg2rad(20.0)) / np.cos(np.deg2rad(22.5)) - 1.0
    assert bound < 0.018
    err = np.abs(o.depth / D - 1.0)
    print("max relative depth error %.4f (bound at 20 degrees %.4f)" % (err.max(), bound))
    assert err.max() <= 0.025
