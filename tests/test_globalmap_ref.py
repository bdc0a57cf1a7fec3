"""tests/globalmap_ref.py against independent statements of the same steps (no GPU): step 3 against the sequential loop of
globalMappingOcTree.cpp:694-704 transcribed with a Python set, steps 5 and 6 against scipy's cKDTree, step 4 against clear + inserts.
The inputs are the synthetic room of globalmap_ref.room()."""
import numpy as np
import pytest
from scipy.spatial import cKDTree

import globalmap_ref as gr

F32 = np.float32
ULP4 = 4 * float(np.finfo(F32).eps)          # "within 4 float ulp", relative


def sequential_insert(occupied, points, q, res, origin=(0.0, 0.0, 0.0)):
    """:694-704, point by point: a point goes in only if its voxel is still empty."""
    r = float(F32(res))
    for p in q:
        v = tuple(int(np.floor((float(p[a]) - origin[a]) / r)) for a in range(3))
        if v not in occupied:
            occupied.add(v)
            points.append(p)


@pytest.mark.parametrize("res", [0.05, 0.3])
def test_insert_equals_the_sequential_loop(res):
    poses, scans = gr.room()
    m = gr.RefMap(res)
    occupied, points = set(), []
    survivors = []
    for T, s in zip(poses, scans):
        survivors.append(len(m.insert(s, T)))
        sequential_insert(occupied, points, gr.transform(T, s), res)
        assert np.array_equal(m.points, np.array(points, F32))
    print("survivors per scan at %.2f m:" % res, survivors, "map", len(m.points))
    assert survivors[0] > 4 * survivors[-1] if res == 0.3 else min(survivors) > 1000        # both thinning regimes do real work


def test_insert_with_a_shifted_origin_and_without_thinning():
    poses, scans = gr.room()
    origin = (0.013, -0.021, 0.004)
    m = gr.RefMap(0.3, origin)
    occupied, points = set(), []
    for T, s in zip(poses[:3], scans[:3]):
        m.insert(s, T)
        sequential_insert(occupied, points, gr.transform(T, s), 0.3, origin)
    assert np.array_equal(m.points, np.array(points, F32))
    assert not np.array_equal(m.points, _room_map(0.3, 3).points)
    e = gr.RefMap(0.0)
    for T, s in zip(poses[:3], scans[:3]):
        e.insert(s, T)
    assert np.array_equal(e.points, np.concatenate([gr.transform(T, s) for T, s in zip(poses[:3], scans[:3])]))


def test_voxel_is_floor_not_truncation():
    p = np.array([[-0.25, 0.25, -0.0], [-0.2500001, 0.2499999, 0.0], [-1e-9, 1e-9, -0.5]], F32)
    assert gr.voxel(p, 0.25).tolist() == [[-1, 1, 0], [-2, 0, 0], [-1, 0, -2]]
    with pytest.raises(ValueError):
        gr.voxel(np.array([[0.0, 0.0, 0.25 * (1 << 20)]], F32), 0.25)
    assert gr.voxel(np.array([[0.0, 0.0, -0.25 * ((1 << 20) - 1)]], F32), 0.25)[0, 2] == -(1 << 20) + 1


_MAPS = {}


def _room_map(res, n_scans=12):
    if (res, n_scans) not in _MAPS:
        poses, scans = gr.room()
        m = gr.RefMap(res)
        for T, s in zip(poses[:n_scans], scans[:n_scans]):
            m.insert(s, T)
        _MAPS[(res, n_scans)] = m
    return _MAPS[(res, n_scans)]


def _query():
    poses, scans = gr.room()
    return scans[5][:400], poses[5]


def test_radius_set_equals_ckdtree():
    m = _room_map(0.05)
    xyz, T = _query()
    q = gr.transform(T, xyz)
    radius = 0.5
    r2 = F32(radius * radius)
    s = gr.sqdist(q, m.points)
    mine = s <= r2
    border = np.abs(s.astype(np.float64) - float(r2)) <= ULP4 * float(r2)
    tree = cKDTree(m.points.astype(np.float64))
    theirs = np.zeros_like(mine)
    for i, js in enumerate(tree.query_ball_point(q.astype(np.float64), radius)):
        theirs[i, js] = True
    n_pairs = int(mine.sum())
    print("pairs in range", n_pairs, "left out", int(border.sum()))
    assert border.sum() <= 1e-3 * n_pairs
    assert np.array_equal(mine & ~border, theirs & ~border)
    if not border.any():
        assert np.array_equal(m.in_radius(xyz, T, radius), theirs.any(axis=0))
    ref, idx = m.reference_radius(xyz, T, radius, 0.3)
    u = int(m.in_radius(xyz, T, radius).sum())
    print("in radius", u, "thinned to", len(idx))
    assert 4 * len(idx) < u and np.all(np.diff(idx) > 0)                                   # the thinning does real work; ascending j
    k = gr.pack(gr.voxel(ref, 0.3))
    assert len(np.unique(k)) == len(k)                                                      # one point per voxel ...
    all_u = np.nonzero(m.in_radius(xyz, T, radius))[0]
    ku = gr.pack(gr.voxel(m.points[all_u], 0.3))
    assert set(k.tolist()) == set(ku.tolist())                                              # ... of every occupied voxel ...
    assert all(j == all_u[ku == kv].min() for j, kv in zip(idx.tolist(), k.tolist()))       # ... the smallest j
    everything, _ = m.reference_radius(xyz, T, radius, 0.0)
    assert len(everything) == u


def test_knn_equals_ckdtree():
    m = _room_map(0.05)
    xyz, T = _query()
    q = gr.transform(T, xyz)
    tree = cKDTree(m.points.astype(np.float64))
    d, j = tree.query(q.astype(np.float64), k=6)
    mine = m.knn(xyz, T, 5, 1.5)
    s = gr.sqdist(q, m.points)
    left_out = 0
    for i in range(len(q)):
        d2 = s[i, j[i]].astype(np.float64)
        if abs(d2[4] - d2[5]) <= ULP4 * d2[5] or np.any(np.abs(d2 - 1.5) <= ULP4 * 1.5):
            left_out += 1
            continue
        expect = sorted(int(v) for v, dd in zip(j[i, :5], s[i, j[i, :5]]) if dd <= F32(1.5))
        assert sorted(mine[i][1].tolist()) == expect, i
    print("queries left out", left_out)
    assert left_out <= 1e-3 * len(q)
    for dd, jj in mine:                                                                      # (d2, j) lexicographic
        assert all((dd[a], jj[a]) < (dd[a + 1], jj[a + 1]) for a in range(len(jj) - 1))
    ref, idx = m.reference_knn(xyz, T, 5, 1.5)
    assert np.array_equal(idx, np.concatenate([jj for _, jj in mine])) and np.array_equal(ref, m.points[idx])
    assert len(np.unique(idx)) < len(idx)                                                    # a map point found from two query points appears twice


def test_hand_over_is_step_one():
    m = _room_map(0.3)
    xyz, T = _query()
    Tinv = np.linalg.inv(T)
    a, ia = m.reference_radius(xyz, T, 0.5, 0.3, T_out=Tinv)
    b, ib = m.reference_radius(xyz, T, 0.5, 0.3)
    assert np.array_equal(ia, ib) and np.array_equal(a, gr.transform(Tinv, b)) and not np.array_equal(a, b)


@pytest.mark.parametrize("res", [0.05, 0.0])
def test_rebuild_equals_clear_and_inserts(res):
    poses, scans = gr.room()
    a, b = gr.RefMap(res), gr.RefMap(res)
    for k, s in enumerate(scans):
        a.add_scan(10 + k, s); b.add_scan(10 + k, s)
    a.insert(scans[0], poses[3])                                                            # something to be forgotten
    moved = [gr.pose(0.01 * k, -0.02 * k, 0.0, 0.001 * k) @ T for k, T in enumerate(poses)]
    keys = [10 + k for k in range(12) if k != 4]
    Ts = [moved[k - 10] for k in keys]
    a.rebuild(keys, Ts)
    for k, T in zip(keys, Ts):
        b.insert_key(k, T)
    assert np.array_equal(a.points, b.points) and len(a.points) > 10000
    more = a.insert(scans[4], moved[4]); b.insert(scans[4], moved[4])
    assert np.array_equal(a.points, b.points) and 0 < len(more)
