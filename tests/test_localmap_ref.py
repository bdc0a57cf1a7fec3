"""tests/localmap_ref.py proves itself (no GPU): the cube of a coordinate with the reference's quirk, the six shifts, the order of the
valid cubes, the publication state machine and the reset of q_wmap_wodom on hand-made cases; a second, independent formulation agrees
with the transcription on raw bytes over a random walk; two mutants each fail a named case."""
import numpy as np
import pytest

import localmap_ref as R

F = np.float32
COORDS = (10.0, float(np.nextafter(10.0, 0.0)), 0.0, -0.0, -1e-30, -10.0, -10.000001, -20.0)
CUBE_OF = (1, 0, 0, 0, -1, -2, -2, -3)                  # relative to the centre
I0 = np.array([0.0, 0.0, 0.0, 1.0])


def index(i, j, k):
    return i + R.W * j + R.W * R.H * k


def one(x, y, z, w=1.0):
    return np.array([[x, y, z, w]], F)


def occupied(m, cls):
    return {e: len(m.cube(cls, e)) for e in range(R.CUBES) if len(m.cube(cls, e))}


# ---- the cube of a coordinate ----------------------------------------------------------------------------------------------------------
def table(half=False, decrement=True):
    xy = [R.cube_index(v, 10.0, 5, half=5.0 if half else 0.0, decrement=decrement) - 5 for v in COORDS]
    z = [R.cube_index(0.5 * v, 5.0, 3, half=2.5 if half else 0.0, decrement=decrement) - 3 for v in COORDS]
    return tuple(xy), tuple(z)


def test_cube_of_a_coordinate_has_the_reference_quirk():
    xy, z = table()
    assert xy == CUBE_OF, xy
    assert z == CUBE_OF, z                                                       # the same pattern in z with 5.0


def test_mutant_half_cube_fails_the_boundary_case():
    """H = half a cube (what the reference's author meant): 9.999... would land in cube 1, not 0."""
    xy, _ = table(half=True)
    assert xy[1] == 1 and xy != CUBE_OF


def test_mutant_truncation_without_decrement_fails_the_small_negative_case():
    xy, _ = table(decrement=False)
    assert xy[4] == 0 and xy[5] == -1 and xy != CUBE_OF                          # -1e-30 -> 0 instead of -1, -10.0 -> -1 instead of -2


def test_the_state_uses_the_same_rule_for_points():
    """Through a whole push, in float32 as the points are: x and z carry the table, y keeps the points in different voxels of cube 0."""
    xs = np.asarray(COORDS, F)                                                    # (the double next below 10.0 is 10.0f; the others survive)
    for make in (R.LocalMapRef, R.LocalMapDict):
        m = make()
        corner = np.array([[v, F(0.5 + 0.3 * n), F(0.5) * v, 7.0] for n, v in enumerate(xs)], F)
        res = m.push(corner, R.empty(), I0, np.zeros(3))
        assert res.n_added == [len(COORDS), 0]
        want = {}
        for v in xs:
            e = index(R.cube_index(np.float64(v), 10.0, 5), 5, R.cube_index(np.float64(F(0.5) * v), 5.0, 3))
            want[e] = want.get(e, 0) + 1
        assert occupied(m, 0) == want
        assert want[index(6, 5, 4)] == 2 and want[index(5, 5, 3)] == 2 and want[index(4, 5, 2)] == 1 and want[index(3, 5, 1)] == 2 and want[index(2, 5, 0)] == 1


# ---- shifts ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("axis, sign", [(a, s) for a in range(3) for s in (1, -1)])
def test_single_shift_in_every_direction(axis, sign):
    m = R.LocalMapRef()
    m.push(one(1.0, 1.0, 1.0), one(2.0, 2.0, 2.0), I0, np.zeros(3))
    assert occupied(m, 0) == {index(5, 5, 3): 1} and occupied(m, 1) == {index(5, 5, 3): 1}
    size = 5.0 if axis == 2 else 10.0
    # up: the centre must fall below 3 (I, J: 5 + int(-2.5) - 1 = 2; K: 3 + int(-0.5) - 1 = 2); down: reach size - 3 (I, J: 5 + 3 = 8; K: 3 + 1 = 4)
    factor = {(0, 1): -2.5, (1, 1): -2.5, (2, 1): -0.5, (0, -1): 3.5, (1, -1): 3.5, (2, -1): 1.5}[(axis, sign)]
    t = np.zeros(3); t[axis] = factor * size
    res = m.push(R.empty(), R.empty(), I0, t)
    want = [0, 0, 0]; want[axis] = sign
    assert res.shift == want
    ijk = [5, 5, 3]; ijk[axis] += sign
    assert occupied(m, 0) == {index(*ijk): 1} and occupied(m, 1) == {index(*ijk): 1}
    cen = [5, 5, 3]; cen[axis] += sign
    assert m.cen == cen


def test_double_shift_and_a_shift_that_discards_occupied_cubes():
    m = R.LocalMapRef()
    m.push(np.concatenate([one(1.0, 1.0, 1.0), one(-41.0, 1.0, 1.0), one(51.0, 1.0, 1.0)]), R.empty(), I0, np.zeros(3))
    assert occupied(m, 0) == {index(5, 5, 3): 1, index(0, 5, 3): 1, index(10, 5, 3): 1}
    res = m.push(R.empty(), R.empty(), I0, np.array([-35.0, 0.0, 0.0]))           # centre int(-3.5) + 5 - 1 = 1: two passes of `while (centerCubeI < 3)`
    assert res.shift == [2, 0, 0] and m.cen == [7, 5, 3]
    assert occupied(m, 0) == {index(7, 5, 3): 1, index(2, 5, 3): 1}              # the cube at i = 10 left the array with its point
    res = m.push(R.empty(), R.empty(), I0, np.array([45.0, 0.0, 0.0]))            # centre 4 + 7 = 11: four passes down
    assert res.shift == [-4, 0, 0] and m.cen == [3, 5, 3]
    assert occupied(m, 0) == {index(3, 5, 3): 1}                                 # i = 2 - 4 < 0 is gone


def test_valid_cube_order_and_clipping():
    v = R.valid_cubes((5, 5, 3))
    assert len(v) == 75
    assert v[:4] == [index(3, 3, 2), index(3, 3, 3), index(3, 3, 4), index(3, 4, 2)]      # k innermost, then j, then i
    assert v[-1] == index(7, 7, 4)
    m = R.LocalMapRef()
    pts_ = np.array([[-15.0, -15.0, -2.0, 1.0], [-15.0, -15.0, 2.0, 2.0], [-15.0, -5.0, -2.0, 3.0], [15.0, 15.0, 2.0, 4.0]], F)
    m.push(pts_, R.empty(), I0, np.zeros(3))
    res = m.push(R.empty(), R.empty(), I0, np.zeros(3))
    assert res.from_map[0][:, 3].tolist() == [1.0, 2.0, 3.0, 4.0]                # concatenated in that order
    assert len(R.valid_cubes((3, 5, 3))) == 75 and len(R.valid_cubes((1, 5, 3))) == 60 and len(R.valid_cubes((5, 5, 0))) == 50


def test_an_invalid_cube_keeps_raw_points_until_it_becomes_valid():
    m = R.LocalMapRef()
    far = np.array([[31.01, 1.0, 1.0, 1.0], [31.31, 1.0, 1.0, 2.0]], F)          # two voxels of 0.2 (the stack keeps both), three cubes from the centre
    m.push(far, R.empty(), I0, np.zeros(3)); m.push(far, R.empty(), I0, np.zeros(3))
    assert m.cube(0, index(8, 5, 3))[:, 3].tolist() == [1.0, 2.0, 1.0, 2.0]
    m.push(R.empty(), R.empty(), I0, np.array([11.0, 0.0, 0.0]))                  # centre 6: i = 8 is valid now
    assert m.cube(0, index(8, 5, 3))[:, 3].tolist() == [1.0, 2.0]                 # each voxel's two arrivals merged, once


# ---- publication -----------------------------------------------------------------------------------------------------------------------
def test_publication_state_machine_over_40_frames():
    m = R.LocalMapRef(publish_frames=12)
    x = lambda k: 0.0 if k < 10 else (5.0 if k < 20 else 7.5)                     # noqa: E731
    published = []
    for k in range(40):
        res = m.push(one(1.0, 1.0, 1.0, float(k)), R.empty(), I0, np.array([x(k), 0.0, 0.0]))
        if res.published is not None:
            published.append(k)
            assert occupied(m, 0) == {} and len(res.published[0]) >= 1
        assert res.frame_count == k + 1
    # 10: the first-frame rule.  NOT 11: while first_odom the last pose follows the current one, so the 5 m step between frames 9 and 10 is
    # not seen.  20: 2.5 m > 2.0.  33: 33 - 20 > 12.
    assert published == [10, 20, 33]


def test_published_map_order_and_sensor_frame():
    m = R.LocalMapRef(publish_first_frame=0)
    q = R.yaw_quat(np.pi / 2); t = np.array([1.0, 2.0, 0.5])
    corner = np.array([[3.0, 0.0, 0.0, 1.0], [-13.0, 0.0, 0.0, 2.0]], F); surf = one(3.0, 0.1, 0.0, 3.0)
    res = m.push(corner, surf, q, t)
    world, sensor = res.published
    assert world[:, 3].tolist() == [2.0, 1.0, 3.0]                                # cube index order, corner then surf per cube
    # the sensor-frame copy gives the stack points back (to float rounding), in the published order
    assert np.allclose(sensor[:, :3], [[-13.0, 0.0, 0.0], [3.0, 0.0, 0.0], [3.0, 0.1, 0.0]], atol=1e-5) and sensor[:, 3].tolist() == [2.0, 1.0, 3.0]
    assert np.array_equal(sensor, R.to_sensor(R.quat_to_R(q), t, world))


def test_wmap_wodom_follows_the_alignment_and_is_reset_by_a_publication():
    m = R.LocalMapRef(publish_first_frame=2)
    rng = np.random.default_rng(5)
    corner = np.concatenate([rng.uniform(-4, 4, (40, 3)), np.ones((40, 1))], axis=1).astype(F)
    surf = np.concatenate([rng.uniform(-4, 4, (200, 3)), np.ones((200, 1))], axis=1).astype(F)
    nudge = lambda fc, fs, sc, ss, q, t, gate: (q, t + np.array([0.25 if gate else 0.0, 0.0, 0.0]), None)      # noqa: E731
    r0 = m.push(corner, surf, I0, np.zeros(3), align=nudge)
    assert r0.aligned == 0 and np.array_equal(m.t_wmap_wodom, np.zeros(3))        # an empty map: the gate fails
    r1 = m.push(corner, surf, I0, np.array([1.0, 0.0, 0.0]), align=nudge)
    assert r1.aligned == 1 and np.array_equal(r1.t, [1.25, 0.0, 0.0]) and np.array_equal(m.t_wmap_wodom, [0.25, 0.0, 0.0])
    r2 = m.push(corner, surf, I0, np.array([2.0, 0.0, 0.0]), align=nudge)         # the guess carries the correction; frame 2 publishes
    assert np.array_equal(r2.t, [2.5, 0.0, 0.0]) and r2.published is not None
    assert np.array_equal(m.q_wmap_wodom, [0.0, 0.0, 0.0, 1.0]) and np.array_equal(m.t_wmap_wodom, np.zeros(3))
    r3 = m.push(corner, surf, I0, np.array([3.0, 0.0, 0.0]), align=nudge)
    assert r3.aligned == 0 and np.array_equal(r3.t, [3.0, 0.0, 0.0])             # emptied cubes: no alignment, the guess is the odometry again


# ---- the second formulation --------------------------------------------------------------------------------------------------------------
def test_dict_formulation_agrees_with_the_transcription_over_a_random_walk():
    a, b = R.LocalMapRef(publish_first_frame=4, publish_frames=6), R.LocalMapDict(publish_first_frame=4, publish_frames=6)
    shifted = set(); published = 0; dropped = 0
    for k, (corner, surf, q, t) in enumerate(R.walk(seed=27, n=30)):
        ra, rb = a.push(corner, surf, q, t), b.push(corner, surf, q, t)
        assert R.state_bytes(a, ra) == R.state_bytes(b, rb), k
        assert a.cen == b.cen
        for ax in range(3):
            if ra.shift[ax]:
                shifted.add((ax, int(np.sign(ra.shift[ax])), abs(ra.shift[ax]) > 1))
        published += ra.published is not None
        dropped += (len(ra.stack[0]) + len(ra.stack[1])) - sum(ra.n_added)
    assert {(ax, s) for ax, s, _ in shifted} == {(ax, s) for ax in range(3) for s in (1, -1)}, shifted      # the walk is worth the comparison
    assert any(multi for _, _, multi in shifted) and published >= 2 and dropped > 0


def test_mutants_fail_the_walk_too():
    """The byte comparison above has teeth: either mutant of the second formulation disagrees with the transcription."""
    for kw in (dict(half_cube=True), dict(decrement=False)):
        a, b = R.LocalMapRef(), R.LocalMapDict(**kw)
        differ = False
        for corner, surf, q, t in R.walk(seed=11, n=6):
            ra, rb = a.push(corner, surf, q, t), b.push(corner, surf, q, t)
            differ = differ or R.state_bytes(a, ra) != R.state_bytes(b, rb)
        assert differ, kw
