"""GPU parity of the Scan Context place recognition (include/vilsc.h) with its numpy restatement (tests/scancontext_ref.py), through the
C-ABI, bit for bit: descriptors, keys, candidate lists, per-entry distances and shifts, and the decision.

Inputs: the device's atan and numpy's may differ in the last bit, which could move a point across a sector edge.  Generated scans are kept
EDGE_MARGIN_DEG = 1e-3 degrees (about 30 float ulps at 360) off every edge by the generator; hand-built points sit on angles far from one.
That is a choice of inputs, not an exclusion of results."""
import hashlib
import math
import os
import subprocess
import sys

import numpy as np
import pytest

import scancontext_ref as ref
from mvil_fusion_amd import lib, scancontext as sc, vgicp
from test_scancontext_ref import one_per_column, pts, scene, scene_config, shifted

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
F32 = np.float32
MODES = (sc.MODE_REFERENCE, sc.MODE_EXHAUSTIVE)


def raw(a):
    return np.ascontiguousarray(a).view(np.uint8)


def same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(raw(a), raw(b))


def cfg_kw(cfg):
    return dict(lidar_height=cfg.lidar_height, max_radius=cfg.max_radius, dist_thres=cfg.dist_thres, search_ratio=cfg.search_ratio,
                num_exclude_recent=cfg.num_exclude_recent, num_candidates=cfg.num_candidates)


def open_pair(so, cfg, max_entries=64, max_points=8192):
    return sc.ScanContext(so, max_entries=max_entries, max_points=max_points, **cfg_kw(cfg)), ref.Database(cfg)


def check_entry(g, o, i, what=""):
    desc, rk, sk = g.read_entry(i)
    assert same(desc, o.desc[i]), what
    assert same(rk, o.ring[i]), what
    assert same(sk, o.sect[i]), what


def check_detect(g, o, mode, n_search=-1, what=""):
    """One detection on both sides, everything compared bit for bit.  Returns the restatement's result."""
    r = g.detect(mode, n_search)
    dist, shift, cand = g.debug_read()
    e = o.detect(mode, n_search)
    assert cand.tolist() == e.candidates.tolist(), what
    assert same(dist, e.dist) and shift.tolist() == e.shift.tolist(), what
    assert same(np.float64(r.min_dist), np.float64(e.min_dist)), (what, r.min_dist, e.min_dist)
    assert (r.nn_idx, r.nn_align, r.loop_id, r.n_searched) == (e.nn_idx, e.nn_align, e.loop_id, e.n_searched), what
    assert same(F32(r.yaw_diff_rad), F32(e.yaw_diff_rad)), what
    return e


@pytest.fixture(scope="module")
def so():
    return lib.load_vilsolve()


# ---- descriptor parity ----------------------------------------------------------------------------------------------------------------------
def hand_built_scan():
    """2000 points of ONE bin, many of them tying for its maximum; random points of every quadrant, a part of them outside the radius;
    points below -1000; the points the contract drops."""
    rng = np.random.default_rng(7)
    tie = np.tile(F32([[10.0, 10.0, 0.0, 0.0]]), (2000, 1)); tie[:, 2] = rng.choice(F32([-3.0, 0.5, 41.25]), 2000); tie[::7, 2] = 41.25
    tie[:, 0] += rng.uniform(-0.2, 0.2, 2000).astype(F32)
    cloud = rng.uniform(-75.0, 75.0, (1500, 4)).astype(F32); cloud[:, 2] = rng.uniform(-4.0, 6.0, 1500)
    low = F32([[20.0, -30.0, -1500.0, 0.0], [20.5, -30.5, -1002.0, 0.0], [-5.0, 40.0, -1001.5, 0.0]])
    body = sc.keep_off_sector_edges(np.concatenate([tie, cloud, low]))
    bad = F32([[np.nan, 1, 1, 0], [1, np.inf, 1, 0], [0, 0, 9, 0], [-0.0, 0.0, 9, 0], [3e38, 3e38, 1, 0], [2, 2, np.nan, 0], [80.0, 0.0, 1.0, 0.0],
               [np.nextafter(F32(80.0), F32(90.0)), 0.0, 50.0, 0.0], [1e-30, 1e-30, 0.75, 0.0], [0.0, -3.0, 1.0, 0.0], [-4.0, 0.0, 1.0, 0.0]])
    out = np.concatenate([bad[:4], body, bad[4:]])
    return out[rng.permutation(len(out))]


def test_descriptor_parity(so):
    scans, _, _ = scene()
    hand = hand_built_scan()
    assert 2500 < len(scans[0]) < 4500 and 3000 < len(hand) < 3600                              # several workgroups of 256
    g, o = open_pair(so, ref.Config())
    cases = [("hand-built", hand), ("one point", pts((3.0, -4.0, 0.5))), ("no point", np.zeros((0, 4), F32)), ("scene scan, radius 80", scans[0]),
             ("dropped only", F32([[np.nan, 0, 0, 0], [0, 0, 1, 0]]))]
    for i, (name, s) in enumerate(cases):
        assert g.push_scan(s) == i == o.push_scan(s)
        check_entry(g, o, i, name)
    assert (o.desc[0] != 0).sum() > 300 and o.desc[0][ref.ring_sector(pts((10.0, 10.0, 0)), o.cfg)[1][0] - 1, 7] == F32(43.25)
    assert (o.desc[1] != 0).sum() == 1 and not o.desc[2].any() and not o.desc[4].any()
    g.close()
    g, o = open_pair(so, scene_config())
    for i, s in enumerate(scans):
        g.push_scan(s); o.push_scan(s)
        check_entry(g, o, i, "keyframe %d" % i)
    perm = np.random.default_rng(3).permutation(len(scans[2]))                                   # the order of the points does not matter
    j = g.push_scan(scans[2][perm])
    assert same(g.read_entry(j)[0], o.desc[2])
    g.close()


# ---- detection parity -------------------------------------------------------------------------------------------------------------------------
def database_descriptors(n=300, seed=11):
    """Generated and hand-built descriptors: the scene's, random dense and sparse ones with both signs, noisy shifted copies of earlier
    ones (near matches), exact duplicates, entries with all-zero columns and an all-zero entry."""
    rng = np.random.default_rng(seed)
    out = [ref.make_descriptor(s, scene_config()) for s in scene()[0]]
    while len(out) < n:
        kind = len(out) % 6
        if kind == 0:
            d = rng.uniform(-2.0, 6.0, (20, 60)).astype(F32)
        elif kind == 1:
            d = np.where(rng.random((20, 60)) < 0.1, rng.uniform(-2.0, 6.0, (20, 60)), 0.0).astype(F32)
        elif kind == 2:
            d = shifted(out[int(rng.integers(0, len(out)))], int(rng.integers(0, 60))) + rng.normal(0, 0.05, (20, 60)).astype(F32)
        elif kind == 3:
            d = shifted(out[int(rng.integers(0, len(out)))], int(rng.integers(0, 60))).copy()
        elif kind == 4:
            d = rng.uniform(0.0, 5.0, (20, 60)).astype(F32); d[:, rng.random(60) < 0.4] = 0.0
        else:
            d = one_per_column(rng.integers(1, 9, 60), int(rng.integers(0, 1 << 30)))
        out.append(np.ascontiguousarray(d, F32))
    if n > 37:
        out[37] = np.zeros((20, 60), F32)
    return out


@pytest.fixture(scope="module")
def big(so):
    """303 entries on both sides, not a multiple of 64, pushed once.  One workgroup of k_sc_cand holds 1024 entries: the candidate search
    across several workgroups is test_candidates_across_workgroups' part."""
    descs = database_descriptors(303)
    g, o = open_pair(so, ref.Config(), max_entries=400, max_points=64)
    for i, d in enumerate(descs):
        assert g.push_descriptor(d) == i == o.push_descriptor(d)
    for i in (0, 37, 150, 302):
        check_entry(g, o, i, "entry %d" % i)
    yield g, o, descs
    g.close()


def test_detection_parity_both_modes(big):
    g, o, descs = big
    rng = np.random.default_rng(5)
    queries = [shifted(descs[40], 13) + rng.normal(0, 0.02, (20, 60)).astype(F32), shifted(descs[3], 50), rng.uniform(-1.0, 4.0, (20, 60)).astype(F32),
               np.where(descs[200] != 0, descs[200] * F32(1.5), 0).astype(F32), shifted(descs[299], 59)]
    found = 0
    for k, q in enumerate(queries):
        g.push_descriptor(q); o.push_descriptor(q)
        for mode in MODES:
            e = check_detect(g, o, mode, what="query %d mode %d" % (k, mode))
            assert e.n_searched == o.count() - 5
            found += e.loop_id >= 0
        e = check_detect(g, o, sc.MODE_REFERENCE, n_search=100, what="query %d, 100 searched" % k)
        assert e.n_searched == 100 and (e.candidates < 100).all()
    assert found >= 6


def test_candidates_across_workgroups(so):
    """1101 entries: two workgroups of k_sc_cand (1024 entries each) and the merge of their lists in k_sc_select.  The query's near copies
    lie in both chunks (indices 7, 500, 1023 | 1024, 1060, 1090), entries 3 and 1030 are IDENTICAL to each other and so are 900 and 1095
    (equal ring-key distances across the chunk border: the smaller index comes first), and ten candidates are taken, more than either
    chunk holds near copies of."""
    rng = np.random.default_rng(21)
    base = rng.uniform(0.0, 5.0, (20, 60)).astype(F32)
    near = lambda amp: shifted(base, int(rng.integers(0, 60))) + rng.normal(0, amp, (20, 60)).astype(F32)
    twin_a, twin_b = near(0.03), near(0.2)
    special = {7: near(0.01), 500: near(0.05), 1023: near(0.02), 1024: near(0.015), 1060: near(0.04), 1090: near(0.025), 3: twin_a, 1030: twin_a, 900: twin_b, 1095: twin_b}
    cfg = ref.Config(num_candidates=10)
    g, o = open_pair(so, cfg, max_entries=1200, max_points=16)
    for i in range(1101):
        d = special[i] if i in special else rng.uniform(0.0, 5.0, (20, 60)).astype(F32)
        g.push_descriptor(d); o.push_descriptor(d)
    q = shifted(base, 11)
    g.push_descriptor(q); o.push_descriptor(q)
    e = check_detect(g, o, sc.MODE_REFERENCE, what="1097 searched")
    assert e.n_searched == 1097 and sorted(e.candidates.tolist()) == sorted(special)             # all ten, from both chunks
    c = e.candidates.tolist()
    assert c.index(3) + 1 == c.index(1030) and c.index(900) + 1 == c.index(1095)                 # ties: the smaller index first
    for n_search in (1025, 1024, 1031, 1101):
        e = check_detect(g, o, sc.MODE_REFERENCE, n_search=n_search, what="%d searched" % n_search)
        assert len(e.candidates) == 10 and {i for i in special if i < n_search} <= set(e.candidates.tolist())
    e = check_detect(g, o, sc.MODE_EXHAUSTIVE, what="exhaustive, 1097 searched")
    assert len(e.dist) == 1097 and e.loop_id in special
    g.close()


def test_ties_go_to_the_first(so):
    d = one_per_column(np.random.default_rng(2).integers(1, 9, 60), 9)
    rng = np.random.default_rng(4)
    g, o = open_pair(so, ref.Config())
    for e in [rng.uniform(0, 4, (20, 60)).astype(F32), d, rng.uniform(0, 4, (20, 60)).astype(F32), d] + [rng.uniform(0, 4, (20, 60)).astype(F32) for _ in range(5)] + [shifted(d, 21)]:
        g.push_descriptor(e); o.push_descriptor(e)
    for mode in MODES:
        e = check_detect(g, o, mode)
        assert (e.nn_idx, e.nn_align, e.min_dist, e.loop_id) == (1, 21, 0.0, 1)                   # entries 1 and 3 are identical
    assert o.detect(sc.MODE_REFERENCE).candidates.tolist()[:2] == [1, 3]
    g.close()


def test_edges(so):
    rng = np.random.default_rng(8)
    d = rng.uniform(0.0, 5.0, (20, 60)).astype(F32)
    holes = rng.uniform(0.0, 5.0, (20, 60)).astype(F32); holes[:, ::3] = 0.0
    g, o = open_pair(so, ref.Config(), max_entries=12, max_points=16)
    for k in range(5):                                                                            # the early return
        e = holes if k == 2 else rng.uniform(0.0, 5.0, (20, 60)).astype(F32)
        g.push_descriptor(e); o.push_descriptor(e)
        for mode in MODES:
            e = check_detect(g, o, mode)
            assert (e.loop_id, e.n_searched, len(e.dist)) == (-1, 0, 0)
    for e in (rng.uniform(0.0, 5.0, (20, 60)).astype(F32), rng.uniform(0.0, 5.0, (20, 60)).astype(F32), rng.uniform(0.0, 5.0, (20, 60)).astype(F32), shifted(d, 9)):
        g.push_descriptor(e); o.push_descriptor(e)
    g.push_descriptor(shifted(d, 30)); o.push_descriptor(shifted(d, 30))                          # entry 9 queries; its match is entry 8
    for mode in MODES:
        assert check_detect(g, o, mode).n_searched == 5                                           # the default hides it: 10 - 5
        assert check_detect(g, o, mode, n_search=9).nn_idx == 8
        assert check_detect(g, o, mode, n_search=8).loop_id != 8                                  # an explicit n_search that hides it
        assert len(check_detect(g, o, mode, n_search=2).dist) == 2                                # fewer than num_candidates
        assert len(check_detect(g, o, mode, n_search=1).dist) == 1
        check_detect(g, o, mode, n_search=10)                                                     # the query itself is searched when the caller asks for it
    q = shifted(holes, 4)
    g.push_descriptor(q); o.push_descriptor(q)                                                    # zero columns on both sides
    for mode in MODES:
        e = check_detect(g, o, mode, n_search=10)
        assert e.nn_idx == 2 and e.nn_align == 4
    zero = np.zeros((20, 60), F32)
    g.push_descriptor(zero); o.push_descriptor(zero)                                              # all-zero query; the database is full now
    for mode in MODES:
        e = check_detect(g, o, mode)
        assert e.min_dist == 10000000.0 and (e.loop_id, e.nn_idx, e.nn_align) == (-1, 0, 0)
    # capacity errors leave the database untouched
    assert g.count() == 12
    before = [g.read_entry(i) for i in range(12)]
    for call in (lambda: g.push_descriptor(d), lambda: g.push_scan(pts((1, 1, 1))), lambda: g.detect(sc.MODE_REFERENCE, 0), lambda: g.detect(sc.MODE_REFERENCE, 13), lambda: g.detect(2),
                 lambda: g.read_entry(12)):
        with pytest.raises(sc.ScanContextError) as err:
            call()
        assert err.value.status == -1
    assert g.count() == 12 and all(same(a, b) for i in range(12) for a, b in zip(before[i], g.read_entry(i)))
    g.reset()
    assert g.count() == 0
    with pytest.raises(sc.ScanContextError) as err:
        g.push_scan(np.zeros((17, 4), F32))                                                       # more than max_points
    assert err.value.status == -1 and g.count() == 0
    assert g.push_descriptor(d) == 0 and same(g.read_entry(0)[0], d)
    g.close()


# ---- the generated trajectory --------------------------------------------------------------------------------------------------------------
def test_scene_property_and_non_default_configuration(so):
    scans, _, rev = scene()
    for cfg in (scene_config(), ref.Config(max_radius=40.0, num_candidates=10, search_ratio=0.2, num_exclude_recent=2, lidar_height=sc.SCENE_LIDAR_HEIGHT)):
        g, o = open_pair(so, cfg)
        extra = database_descriptors(30, seed=12)[11:]
        for i, s in enumerate(scans):
            assert g.push_scan(s) == o.push_scan(s)
            check_entry(g, o, g.count() - 1)
            er = check_detect(g, o, sc.MODE_REFERENCE); ex = check_detect(g, o, sc.MODE_EXHAUSTIVE)
            assert er.n_searched == ex.n_searched == max(0, i + 1 - cfg.num_exclude_recent) * (i + 1 >= cfg.num_exclude_recent + 1)
            assert ex.min_dist <= er.min_dist
            for slot, c in enumerate(er.candidates):                                              # a pair scored in both modes: the same bits
                if er.dist[slot] != 10000000.0:                                                   # no shift won: nothing was scored below 10000000
                    assert same(np.float64(er.dist[slot]), np.float64(ex.all_shifts[c, er.shift[slot]]))
                assert ex.dist[c] <= er.dist[slot]
            if er.n_searched and cfg.max_radius == sc.SCENE_RADIUS:
                assert er.loop_id == ex.loop_id == rev[i]
        for d in extra:                                                                           # more entries than num_candidates = 10
            g.push_descriptor(d); o.push_descriptor(d)
        for mode in MODES:
            e = check_detect(g, o, mode)
            assert len(e.dist) == (min(cfg.num_candidates, e.n_searched) if mode == sc.MODE_REFERENCE else e.n_searched)
        g.close()


def test_chain_detect_then_verify(so):
    """vsc_push_scan per keyframe, vsc_detect finds each revisit and rejects each first visit; for one found pair the existing vgicp wrapper,
    started from the yaw nn_align implies (vilsc.h, SIGN OF nn_align) and no translation, recovers the known relative pose to the tolerance
    test_gpu_vgicp.py uses for its pair."""
    scans, poses, rev = scene()
    g = sc.ScanContext(so, max_entries=16, max_points=8192, **cfg_kw(scene_config()))
    hits = {}
    for i, s in enumerate(scans):
        g.push_scan(s)
        r = g.detect(sc.MODE_REFERENCE)
        if i >= 5:
            assert r.loop_id == rev[i], (i, r.loop_id, r.min_dist)
            if r.loop_id >= 0:
                hits[i] = r
    g.close()
    assert sorted(hits) == [7, 8, 9, 10]
    q = 7; e = hits[q].loop_id                                                                    # yard 3: walls 7.6 m away on all sides
    (Rq, tq), (Re, te) = poses[q], poses[e]
    T_true = np.eye(4); T_true[:3, :3] = Re.T @ Rq; T_true[:3, 3] = Re.T @ (tq - te)            # p_entry = T_true p_query
    guess = np.eye(4); guess[:3, :3] = sc.rot_z(-float(hits[q].yaw_diff_rad))
    assert abs(-hits[q].yaw_diff_rad - sc.yaw_of_align(hits[q].nn_align)) < 1e-6
    v = vgicp.Vgicp(so, "vgicp_")
    v.set_target(scans[e][:, :3], None, 0.5); v.set_source(scans[q][:, :3], None)
    T, s = v.align(guess)
    v.close()
    print("yaw of the guess %.2f deg, true %.2f deg; |dt| %s" % (math.degrees(math.atan2(guess[1, 0], guess[0, 0])), math.degrees(math.atan2(T_true[1, 0], T_true[0, 0])),
                                                                  np.abs(T[:3, 3] - T_true[:3, 3])))
    assert s.converged == 1
    assert np.abs(T[:3, 3] - T_true[:3, 3]).max() < 0.03
    # the rotation too: an angle error of a displaces the walls, 7.6 m away, by 7.6 a; the same 0.03 m gives 0.004 rad.  The guess itself
    # is off by up to half a sector (0.05 rad), and a wrong sign of nn_align by 3 rad
    dR = T[:3, :3].T @ T_true[:3, :3]
    angle = math.acos(min(1.0, max(-1.0, (np.trace(dR) - 1.0) / 2.0)))
    print("rotation error %.2e rad" % angle)
    assert angle < 0.03 / 7.6


# ---- determinism ----------------------------------------------------------------------------------------------------------------------------
def snapshot(so):
    """A digest of every result of a fixed sequence of pushes and detections (also run by scancontext_child.py in a fresh process)."""
    scans, _, _ = scene()
    h = hashlib.sha256()
    g = sc.ScanContext(so, max_entries=64, max_points=8192, **cfg_kw(scene_config()))
    for i, s in enumerate(list(scans) + database_descriptors(40, seed=13)[11:]):
        g.push_scan(s) if s.shape[1] == 4 else g.push_descriptor(s)
        for a in g.read_entry(i):
            h.update(raw(a).tobytes())
        for mode in MODES:
            r = g.detect(mode)
            h.update(bytes(r))
            for a in g.debug_read():
                h.update(raw(a).tobytes())
    g.close()
    return h.hexdigest()


def test_determinism(so):
    a = snapshot(so)
    assert snapshot(so) == a
    out = subprocess.run([sys.executable, os.path.join(HERE, "scancontext_child.py")], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr[-2000:]
    assert "digest " + a in out.stdout, out.stdout[-500:]


def test_profile_counts_every_kernel(so):
    scans, _, _ = scene()
    g = sc.ScanContext(so, max_entries=16, max_points=8192, **cfg_kw(scene_config()))
    g.profile_enable(True); g.profile_read()
    for s in scans[:7]:
        g.push_scan(s)
    g.detect(sc.MODE_REFERENCE); g.detect(sc.MODE_EXHAUSTIVE)
    prof = g.profile_read()
    g.profile_enable(False); g.close()
    assert sorted(prof) == sorted(sc.KERNELS)
    assert [prof[k][0] for k in sc.KERNELS] == [7, 7, 1, 1, 2, 2] and all(ms > 0 for _, ms in prof.values()), prof
