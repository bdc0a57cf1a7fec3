"""Pins tests/scancontext_ref.py, the numpy restatement of include/vilsc.h's arithmetic contract, on hand-built cases, and checks that the
generated scene of mvil_fusion_amd.scancontext separates revisits from first visits with room to spare.  No GPU."""
import functools
import math

import numpy as np

import scancontext_ref as ref
from mvil_fusion_amd import scancontext as sc

F32 = np.float32


def pts(*rows):
    return np.array([list(r) + [0.0] for r in rows], F32)


def occupied(desc):
    return sorted((int(r) + 1, int(c) + 1) for r, c in zip(*np.nonzero(desc)))


@functools.lru_cache(maxsize=None)
def scene(seed=0):
    """(scans, poses, revisit_of) of the generated trajectory; shared with the GPU tests, never modified."""
    return sc.make_scene(seed)


def scene_config(**kw):
    return ref.Config(max_radius=sc.SCENE_RADIUS, lidar_height=sc.SCENE_LIDAR_HEIGHT, **kw)


# ---- step 1 ---------------------------------------------------------------------------------------------------------------------------
def test_one_point_per_branch_of_xy2theta():
    th = ref.xy2theta(F32([1, -1, -1, 1]), F32([1, 1, -1, -1]))
    assert th.dtype == F32 and th.tolist() == [45.0, 135.0, 225.0, 315.0]
    cfg = ref.Config()
    for (x, y), sector in zip([(1, 1), (-1, 1), (-1, -1), (1, -1)], [8, 23, 38, 53]):          # ceil(theta / 6)
        d = ref.make_descriptor(pts((x, y, 0.5)), cfg)
        assert occupied(d) == [(1, sector)] and d[0, sector - 1] == F32(2.5)
    assert ref.xy2theta(F32([0.0]), F32([2.0]))[0] == 90.0 and ref.xy2theta(F32([0.0]), F32([-2.0]))[0] == 270.0


def test_theta_zero_is_clamped_to_sector_one():
    assert ref.xy2theta(F32([3.0]), F32([0.0]))[0] == 0.0                                     # ceil gives 0
    assert occupied(ref.make_descriptor(pts((3.0, 0.0, 1.0)), ref.Config())) == [(1, 1)]


def test_ring_edges():
    cfg = ref.Config()
    assert occupied(ref.make_descriptor(pts((80.0, 0.0, 1.0)), cfg)) == [(20, 1)]             # exactly max_radius
    beyond = np.nextafter(F32(80.0), F32(100.0))
    assert not ref.make_descriptor(pts((beyond, 0.0, 1.0)), cfg).any()                        # one ulp beyond: skipped
    assert occupied(ref.make_descriptor(pts((1e-30, 1e-30, 1.0)), cfg)) == [(1, 8)]           # range underflows to 0: ceil gives 0, ring 1
    assert occupied(ref.make_descriptor(pts((4.0, 0.0, 1.0), (4.0000005, 0.0, 1.0)), cfg)) == [(1, 1), (2, 1)]    # the edge belongs to the inner ring
    assert occupied(ref.make_descriptor(pts((30.0, 0.0, 1.0)), ref.Config(max_radius=40.0))) == [(15, 1)]


def test_minus_1000_rule_and_maximum():
    cfg = ref.Config()
    d = ref.make_descriptor(pts((1, 1, -1002.0), (-1, 1, -2002.0), (-1, -1, -1001.0), (1, -1, 0.25), (1, -1, 3.0), (1, -1, -7.0)), cfg)
    assert d[0, 7] == 0.0 and d[0, 22] == 0.0                                                 # exactly -1000, and below it
    assert d[0, 37] == F32(-999.0) and d[0, 52] == F32(5.0)
    assert occupied(d) == [(1, 38), (1, 53)]


def test_dropped_points_and_nan_height():
    cfg = ref.Config()
    bad = pts((np.nan, 1, 1), (1, np.inf, 1), (0.0, 0.0, 5.0), (-0.0, 0.0, 5.0), (3e38, 3e38, 1))
    assert not ref.make_descriptor(bad, cfg).any()
    d = ref.make_descriptor(pts((1, 1, np.nan), (1, 1, 0.5), (1, 1, np.nan)), cfg)            # a NaN z' never wins
    assert occupied(d) == [(1, 8)] and d[0, 7] == F32(2.5)
    assert not ref.make_descriptor(np.zeros((0, 4), F32), cfg).any()


# ---- steps 2 and 3 ----------------------------------------------------------------------------------------------------------------------
def test_keys():
    d = np.zeros((20, 60), F32); d[2, :] = 3.0; d[5, 7] = 4.0
    rk, sk, nm = ref.make_keys(d)
    assert rk.dtype == F32 and rk[2] == 3.0 and rk[5] == F32(4.0 / 60.0) and sk[7] == 7.0 / 20.0 and sk[8] == 3.0 / 20.0 and nm[7] == 5.0 and nm[0] == 3.0


def test_candidates_are_ordered_by_distance_then_index():
    keys = np.zeros((6, 20), F32)
    keys[0, 0] = 2; keys[1, 3] = 1; keys[2, 0] = 1; keys[4, 19] = 1; keys[3, 0] = np.nan
    q = np.zeros(20, F32)
    assert ref.candidates(keys, q, 6, 4).tolist() == [5, 1, 2, 4]                              # 0, then three at distance 1 by index
    assert ref.candidates(keys, q, 6, 16).tolist() == [5, 1, 2, 4, 0, 3]                       # the NaN last
    assert ref.candidates(keys, q, 2, 3).tolist() == [1, 0]                                    # n_search < num_candidates


# ---- steps 4 and 5 ----------------------------------------------------------------------------------------------------------------------
def one_per_column(values, seed):
    """a descriptor with ONE occupied ring per column: norms and cosines are exact"""
    rng = np.random.default_rng(seed)
    d = np.zeros((20, 60), F32)
    d[rng.integers(0, 20, 60), np.arange(60)] = values
    return d


def shifted(d, k):
    return np.roll(d, k, axis=1)                                                              # column j of the result is column (j - k) mod 60 of d


def detect_pair(entry, query, mode, **kw):
    db = ref.Database(ref.Config(num_exclude_recent=1, **kw))
    db.push_descriptor(entry); db.push_descriptor(query)
    return db.detect(mode)


def test_shifted_descriptor_scores_exactly_zero_at_its_shift():
    d = one_per_column(np.random.default_rng(1).integers(1, 10, 60), 2)
    for k in (0, 1, 20, 59):
        r = detect_pair(d, shifted(d, k), ref.MODE_EXHAUSTIVE)
        assert r.min_dist == 0.0 and r.nn_align == k and r.loop_id == 0 and r.n_searched == 1
        assert r.yaw_diff_rad == F32(np.float64(F32(k * 6.0)) * math.pi / 180.0)
        # distinct sector keys: the pre-alignment lands on k itself and REFERENCE mode finds it too, with the same bits
        r2 = detect_pair(d, shifted(d, k), ref.MODE_REFERENCE)
        assert r2.min_dist == 0.0 and r2.nn_align == k


def test_reference_mode_misses_a_shift_the_sector_key_does_not_see():
    d = one_per_column(5.0, 3)                                                                # every column mean is 0.25: the sector key is flat
    k = 20
    ex = detect_pair(d, shifted(d, k), ref.MODE_EXHAUSTIVE)
    assert ex.min_dist == 0.0 and ex.nn_align == k
    r = detect_pair(d, shifted(d, k), ref.MODE_REFERENCE)                                    # pre-alignment: all norms 0, the first wins: a = 0, shifts 57 .. 3
    assert r.nn_align in (57, 58, 59, 0, 1, 2, 3) and r.min_dist > 0.5 and r.loop_id == -1
    assert r.min_dist == ex.all_shifts[0, r.nn_align]                                        # the same triple, the same bits
    wide = detect_pair(d, shifted(d, k), ref.MODE_REFERENCE, search_ratio=0.7)               # R = 21 reaches it
    assert wide.min_dist == 0.0 and wide.nn_align == k


def test_all_zero_query_and_zero_columns():
    d = one_per_column(4.0, 4)
    r = detect_pair(d, np.zeros((20, 60), F32), ref.MODE_EXHAUSTIVE)
    assert r.min_dist == 10000000.0 and r.loop_id == -1 and r.nn_idx == 0 and r.nn_align == 0 and np.isnan(r.all_shifts).all()
    r = detect_pair(d, np.zeros((20, 60), F32), ref.MODE_REFERENCE)
    assert r.min_dist == 10000000.0 and r.loop_id == -1
    half = d.copy(); half[:, 30:] = 0.0                                                       # zero columns are not counted
    r = detect_pair(d, half, ref.MODE_EXHAUSTIVE)
    assert r.min_dist == 0.0 and r.nn_align == 0


def test_early_return_and_n_search():
    db = ref.Database(ref.Config())
    d = one_per_column(np.arange(1, 61), 5)
    for i in range(5):
        db.push_descriptor(shifted(d, i))
        r = db.detect()
        assert (r.loop_id, r.n_searched, float(r.yaw_diff_rad), len(r.dist)) == (-1, 0, 0.0, 0)
    db.push_descriptor(shifted(d, 7))
    r = db.detect()
    assert r.n_searched == 1 and r.candidates.tolist() == [0] and r.loop_id == 0 and r.nn_align == 7
    r = db.detect(ref.MODE_EXHAUSTIVE, n_search=3)
    assert r.n_searched == 3 and r.candidates.tolist() == [0, 1, 2] and r.nn_idx == 0 and r.shift.tolist() == [7, 6, 5]   # ties: the smaller index


def test_radius_rounds_half_up():
    assert ref.Config().radius == 3 and ref.Config(search_ratio=0.2).radius == 6 and ref.Config(search_ratio=0.05).radius == 2 and ref.Config(search_ratio=0.0).radius == 0


# ---- the generated scene ------------------------------------------------------------------------------------------------------------------
def test_generated_scans_keep_off_the_sector_edges():
    scans, _, _ = scene()
    for s in scans:
        assert s.dtype == F32 and s.shape[1] == 4 and 2000 < len(s) < 5000
        th = ref.xy2theta(s[:, 0], s[:, 1]).astype(np.float64)
        assert (np.abs(th / 6.0 - np.round(th / 6.0)) * 6.0 >= sc.EDGE_MARGIN_DEG).all()
        assert np.array_equal(th.astype(F32), sc.theta_deg(s[:, 0], s[:, 1]))


def test_scene_separates_revisits_from_first_visits():
    """Every revisit scores below half of dist_thres against its first visit, every first visit above one and a half times it -- in
    both modes -- and the column shift gives the yaw between the two visits to within a sector (vilsc.h, SIGN OF nn_align).  With the
    reference's num_exclude_recent = 5 only keyframes 5 and 6 are first visits that are searched for at all; with num_exclude_recent = 1
    keyframes 1 .. 6 are, against up to six stored places."""
    scans, poses, rev = scene()
    assert sum(r >= 0 for r in rev) == 4
    for exclude, n_first in ((5, 2), (1, 6)):
        for mode in (ref.MODE_REFERENCE, ref.MODE_EXHAUSTIVE):
            db = ref.Database(scene_config(num_exclude_recent=exclude))
            seen = {"first": 0, "revisit": 0}
            for i, s in enumerate(scans):
                db.push_scan(s)
                r = db.detect(mode)
                if r.n_searched == 0:
                    assert i < exclude
                    continue
                assert r.n_searched == i + 1 - exclude
                print("exclude %d mode %d keyframe %d revisit_of %d: min_dist %.4f nn_idx %d nn_align %d" % (exclude, mode, i, rev[i], r.min_dist, r.nn_idx, r.nn_align))
                if rev[i] >= 0:
                    seen["revisit"] += 1
                    assert r.min_dist < 0.5 * db.cfg.dist_thres and r.loop_id == rev[i]
                    yaw = lambda R: math.atan2(R[1, 0], R[0, 0])
                    err = (yaw(poses[i][0]) - yaw(poses[rev[i]][0]) - sc.yaw_of_align(r.nn_align) + math.pi) % (2 * math.pi) - math.pi
                    assert abs(err) <= math.radians(3.5), math.degrees(err)
                else:
                    seen["first"] += 1
                    assert r.min_dist > 1.5 * db.cfg.dist_thres and r.loop_id == -1
            assert seen == {"first": n_first, "revisit": 4}
