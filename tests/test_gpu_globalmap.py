"""include/vilgmap.h on the GPU against tests/globalmap_ref.py, bit for bit: points, their order, indices and counts.  Integer and selection
logic has no tolerance.  The inputs are the synthetic room of globalmap_ref.room() and small exact constructions."""
import ctypes as C
import hashlib
import os
import subprocess
import sys

import numpy as np
import pytest

import globalmap_ref as gr
from mvil_fusion_amd import globalmap, lib, loopverify, posegraph, vgicp

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
F32 = np.float32
I4 = np.eye(4)
SMALL = dict(max_map_points=1 << 15, max_scan_points=2048, max_keys=16, max_keyed_points=1 << 15, max_ref_points=1 << 14)
_FP, _DP, _IP = C.POINTER(C.c_float), C.POINTER(C.c_double), C.POINTER(C.c_int32)


@pytest.fixture(scope="module")
def so():
    return lib.load_vilsolve()


def pair(so, res=0.05, origin=(0.0, 0.0, 0.0), **kw):
    """(device map, restatement) with the same configuration"""
    return globalmap.GlobalMap(so, **dict(SMALL, map_resolution=res, origin=origin, **kw)), gr.RefMap(res, origin)


def same(g, r):
    p = g.points()
    assert g.size()[0] == len(r.points) and p.tobytes() == r.points.tobytes(), (g.size(), len(r.points))


def both_insert(g, r, xyz, T=I4):
    g.insert(xyz, T); r.insert(xyz, T)
    same(g, r)


def filled_room(so, res, n_scans=12):
    poses, scans = gr.room()
    g, r = pair(so, res)
    for T, s in zip(poses[:n_scans], scans[:n_scans]):
        g.insert(s, T); r.insert(s, T)
    same(g, r)
    return g, r


# ---- 1. insert ------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("res", [0.05, 0.3])
def test_room_scans_after_every_insert(so, res):
    poses, scans = gr.room()
    g, r = pair(so, res)
    for T, s in zip(poses, scans):
        both_insert(g, r, s, T)
    print("map at %.2f m: %d points" % (res, len(r.points)))
    g.close()


def test_small_odd_inputs_duplicates_and_no_thinning(so):
    rng = np.random.default_rng(3)
    g, r = pair(so, 0.05)
    for n in (1, 63, 64, 65, 257):
        both_insert(g, r, rng.uniform(-0.4, 0.4, (n, 3)).astype(F32), gr.pose(0.1, 0.2, 0.3, 0.4))
    assert len(r.points) < 1 + 63 + 64 + 65 + 257                                         # some voxels were taken already
    s = rng.uniform(-3, 3, (300, 3)).astype(F32)
    both_insert(g, r, np.concatenate([s, s[::-1], s[:7]]))                                # a scan that holds its points twice and more
    g.close()
    g, r = pair(so, 0.0)
    both_insert(g, r, np.concatenate([s, s]), gr.pose(1, 2, 3, 0.5))
    both_insert(g, r, s[:65])
    assert g.size()[0] == 665
    g.close()


@pytest.mark.parametrize("res", [0.25, 0.5])
def test_points_on_voxel_faces_on_both_sides_of_zero(so, res):
    t = np.arange(-6, 7) * (res / 2)                                                      # faces and centres, exact
    grid = np.array([[x, y, z] for x in t for y in t for z in t[4:9]], F32)
    up, down = np.nextafter(grid, F32(np.inf)), np.nextafter(grid, F32(-np.inf))
    g, r = pair(so, res)
    for pts in (grid[::-1], up, down):
        both_insert(g, r, pts)
    assert gr.voxel(np.array([[-res, -0.0, res]], F32), res).tolist() == [[-1, 0, 1]]
    g.close()
    g, r = pair(so, res, origin=(0.125, -0.0625, 1.0))                                    # the faces move with the anchor
    for pts in (grid, up, down):
        both_insert(g, r, pts)
    g.close()


def test_whole_equals_halves_and_runs_repeat(so):
    poses, scans = gr.room()
    a, _ = pair(so, 0.05)
    b, _ = pair(so, 0.05)
    a.insert(scans[0], poses[0]); b.insert(scans[0], poses[0])
    a.insert(scans[1], poses[1])
    b.insert(scans[1][:700], poses[1]); b.insert(scans[1][700:], poses[1])
    assert a.points().tobytes() == b.points().tobytes()
    a.close(); b.close()


def run_digest(so):
    """Inserts, both references and a rebuild on the room: the digest of every output."""
    poses, scans = gr.room()
    g = globalmap.GlobalMap(so, **dict(SMALL, map_resolution=0.05))
    h = hashlib.sha256()
    for k, (T, s) in enumerate(zip(poses[:6], scans[:6])):
        g.add_scan(k, s); g.insert_key(k, T)
    h.update(g.points().tobytes())
    for mode in ("radius", "knn"):
        x, i = g.reference(scans[3][:400], poses[3], T_out=np.linalg.inv(poses[3]), mode=mode)
        h.update(x.tobytes()); h.update(i.tobytes())
    g.rebuild([0, 2, 3, 5], [poses[1], poses[2], poses[3], poses[4]])
    h.update(g.points().tobytes())
    g.close()
    return h.hexdigest()


def test_bit_reproducible_across_runs_and_processes(so):
    a = run_digest(so)
    assert run_digest(so) == a
    out = subprocess.run([sys.executable, os.path.join(HERE, "globalmap_child.py")], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    child = [l for l in out.stdout.splitlines() if l.startswith("digest ")]
    assert child == ["digest " + a], (child, a)


def home_slot(c, slots):
    """The table's home slot of voxel c as include/vilgmap.h states it."""
    key = ((c[0] + (1 << 20)) << 42) | ((c[1] + (1 << 20)) << 21) | (c[2] + (1 << 20))
    return (((key * 0x9E3779B97F4A7C15) & ((1 << 64) - 1)) >> 32) & (slots - 1)


def test_full_table_with_long_wrapping_probe_chains(so):
    """512 voxels whose home slots are the last 24 of the 1024: every chain runs over the table's end.  Then the map is full."""
    cells = [(x, y, z) for x in range(-20, 20) for y in range(-20, 20) for z in range(-20, 20)]
    cells = [c for c in cells if home_slot(c, 1024) >= 1000][:512]
    assert len(cells) == 512
    pts = ((np.array(cells, np.float64) + 0.5) * 0.25).astype(F32)
    g, r = pair(so, 0.25, max_map_points=512, max_scan_points=512)
    for a, b in ((0, 200), (200, 400), (400, 512)):
        both_insert(g, r, pts[a:b])
    assert g.size()[0] == 512
    x, i = g.reference(pts[:64], I4, mode="radius", radius=0.3, ref_resolution=0.0)
    rx, ri = r.reference_radius(pts[:64], I4, 0.3, 0.0)
    assert np.array_equal(i, ri) and x.tobytes() == rx.tobytes()
    for extra in (pts[:1], np.array([[100.0, 100.0, 100.0]], F32)):                       # taken or free voxel: the count before thinning decides
        with pytest.raises(globalmap.GlobalMapError) as e:
            g.insert(extra, I4)
        assert e.value.status == -7
        same(g, r)
    g.clear(); r.clear()
    both_insert(g, r, pts[::-1])                                                          # the emptied table takes the same chains again
    g.close()


# ---- 2. rebuild -----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("res", [0.05, 0.0])
def test_rebuild(so, res):
    poses, scans = gr.room()
    g, r = pair(so, res)
    h, _ = pair(so, res)
    for k, s in enumerate(scans[:8]):
        g.add_scan(10 + k, s); h.add_scan(10 + k, s); r.add_scan(10 + k, s)
    assert g.size() == (0, 8, 8 * 1500)
    both_insert(g, r, scans[9], poses[9])                                                  # something to be forgotten
    moved = [gr.pose(0.01 * k, -0.02 * k, 0.0, 0.001 * k) @ T for k, T in enumerate(poses)]
    keys = list(range(10, 18))
    g.rebuild(keys, moved[:8]); r.rebuild(keys, moved[:8])
    same(g, r)
    for k in keys:
        h.insert_key(k, moved[k - 10])
    assert h.points().tobytes() == g.points().tobytes()
    both_insert(g, r, scans[8], moved[8])                                                  # the table really was emptied, and filled again
    q, T = scans[8][:300], moved[8]
    x, i = g.reference(q, T, mode="radius")
    rx, ri = r.reference_radius(q, T)
    assert np.array_equal(i, ri) and x.tobytes() == rx.tobytes() and len(i) > 100
    sub = [10, 13, 14, 17]                                                                 # a subset of the keys
    g.rebuild(sub, [poses[k - 10] for k in sub]); r.rebuild(sub, [poses[k - 10] for k in sub])
    same(g, r)
    assert g.size()[1:] == (8, 8 * 1500)
    g.close(); h.close()


# ---- 3. reference, radius mode ----------------------------------------------------------------------------------------------------------------------------
def check_radius(g, r, q, T, T_out=None, **kw):
    x, i = g.reference(q, T, T_out=T_out, mode="radius", **kw)
    rx, ri = r.reference_radius(q, T, kw.get("radius", 0.5), kw.get("ref_resolution", 0.3), T_out)
    assert np.array_equal(i, ri), (len(i), len(ri))
    assert x.tobytes() == rx.tobytes()
    return i


def test_radius_reference_on_the_room(so):
    poses, scans = gr.room()
    g, r = filled_room(so, 0.05)
    q, T = scans[5][:400], poses[5]
    n_thin = len(check_radius(g, r, q, T))
    n_all = len(check_radius(g, r, q, T, ref_resolution=0.0))
    print("in radius %d, thinned to %d" % (n_all, n_thin))
    assert n_all > 4 * n_thin > 0
    check_radius(g, r, q, T, T_out=np.linalg.inv(T))
    check_radius(g, r, q, T, radius=0.2, ref_resolution=0.11)
    check_radius(g, r, scans[7][:65], poses[7], radius=1.3, ref_resolution=0.3)           # cell edge 2 m
    assert len(check_radius(g, r, q, gr.pose(500.0, 0.0, 0.0, 0.0))) == 0                  # a query far outside
    both_insert(g, r, scans[3][:500], gr.pose(0.02, 0.0, 0.01, 0.0) @ poses[3])            # the search grid follows the map
    check_radius(g, r, q, T)
    g.close()
    g, r = pair(so, 0.05)
    assert len(check_radius(g, r, q, T)) == 0                                              # an empty map
    g.close()


def lattice_map(so):
    """The 27 points of a 3 x 3 x 3 unit lattice, each twice (point k and k + 27 are equal), and one point a hair below zero."""
    lat = np.array([[x, y, z] for x in range(3) for y in range(3) for z in range(3)], F32)
    g, r = pair(so, 0.0)
    both_insert(g, r, np.concatenate([lat, lat, np.array([[-1e-10, 5.0, 5.0]], F32)]))
    return g, r


def test_radius_reference_exactly_on_the_threshold(so):
    g, r = lattice_map(so)
    centres = np.array([[x + 0.5, y + 0.5, z + 0.5] for x in range(2) for y in range(2) for z in range(2)], F32)
    edges = np.array([[0.5, 0, 0], [1, 1.5, 2], [2, 2, 0.5], [1.5, 1, 1]], F32)
    r75 = float(np.sqrt(0.75))
    assert F32(r75 * r75) == F32(0.75)
    i = check_radius(g, r, centres[:1], I4, radius=r75, ref_resolution=0.0)
    assert i.tolist() == [0, 1, 3, 4, 9, 10, 12, 13, 27, 28, 30, 31, 36, 37, 39, 40]        # d2 = 0.75 is in range, both copies
    assert len(check_radius(g, r, centres[:1], I4, radius=0.866, ref_resolution=0.0)) == 0
    i = check_radius(g, r, edges, I4, radius=0.5, ref_resolution=0.0)                     # d2 = 0.25 = the threshold
    assert len(i) == 16
    assert len(check_radius(g, r, edges, I4, radius=0.4999999, ref_resolution=0.0)) == 0
    i = check_radius(g, r, centres, I4, radius=r75, ref_resolution=1.0)                   # lattice points lie on voxel faces; of two copies the first
    assert i.tolist() == list(range(27))
    i = check_radius(g, r, centres, I4, radius=r75, ref_resolution=2.0)
    assert i.tolist() == [0, 2, 6, 8, 18, 20, 24, 26]
    # the query's box reaches over a cell boundary that the rounded difference does not see: 0.5 - (-1e-10) rounds to 0.5
    i = check_radius(g, r, np.array([[0.5, 5.0, 5.0]], F32), I4, radius=0.5, ref_resolution=0.0)
    assert i.tolist() == [54]
    g.close()


# ---- 4. reference, kNN mode -------------------------------------------------------------------------------------------------------------------------------
def check_knn(g, r, q, T, k=5, max_dist=1.5, T_out=None):
    x, i = g.reference(q, T, T_out=T_out, mode="knn", k=k, max_dist=max_dist)
    rx, ri = r.reference_knn(q, T, k, max_dist, T_out)
    assert np.array_equal(i, ri), (len(i), len(ri))
    assert x.tobytes() == rx.tobytes()
    return i


def test_knn_reference_on_the_room(so):
    poses, scans = gr.room()
    g, r = filled_room(so, 0.0, n_scans=6)                                                  # the IkdTree variant keeps every point
    q, T = scans[4][:400], poses[4]
    i = check_knn(g, r, q, T)
    assert len(i) == 5 * 400 and len(np.unique(i)) < len(i)                                # a map point found from two query points appears twice
    check_knn(g, r, q[:65], T, k=1, T_out=np.linalg.inv(T))
    check_knn(g, r, q[:65], T, k=64, max_dist=0.3)
    i = check_knn(g, r, q[:130], T, k=5, max_dist=0.004)                                   # fewer than k in range
    assert 0 < len(i) < 5 * 130
    assert len(check_knn(g, r, q[:10], gr.pose(500.0, 0.0, 0.0, 0.0))) == 0
    g.close()


def test_knn_reference_ties_and_threshold(so):
    g, r = lattice_map(so)
    centre = np.array([[0.5, 0.5, 0.5]], F32)
    assert check_knn(g, r, centre, I4, k=5, max_dist=0.75).tolist() == [0, 1, 3, 4, 9]      # sixteen candidates tie at d2 = max_dist: the smallest j
    assert len(check_knn(g, r, centre, I4, k=5, max_dist=0.7499999)) == 0
    assert check_knn(g, r, centre, I4, k=64, max_dist=0.75).tolist() == [0, 1, 3, 4, 9, 10, 12, 13, 27, 28, 30, 31, 36, 37, 39, 40]
    edge = np.array([[0.5, 0, 0], [0.5, 0, 0]], F32)
    assert check_knn(g, r, edge, I4, k=5, max_dist=0.25).tolist() == [0, 9, 27, 36] * 2     # fewer than k, the same points for both queries
    assert len(check_knn(g, r, edge, I4, k=5, max_dist=0.2)) == 0
    assert check_knn(g, r, np.array([[1, 1, 1]], F32), I4, k=3, max_dist=1.0).tolist() == [13, 40, 4]
    g.close()


# ---- 5. errors ------------------------------------------------------------------------------------------------------------------------------------------------
def raw_reference(g, q, T, options, cap):
    """vgmap_reference with sentinel-filled output buffers: (status, n_ref, xyz, idx)"""
    q = np.ascontiguousarray(q, F32); T = np.ascontiguousarray(T, np.float64)
    x = np.full((cap, 3), -7.0, F32); i = np.full(cap, -7, np.int32); n = C.c_int32(-7)
    f = g.lib.vgmap_reference; f.restype = C.c_int
    st = f(g.ctx, C.c_int32(len(q)), q.ctypes.data_as(_FP), T.ctypes.data_as(_DP), C.byref(options), C.cast(None, _DP), C.byref(n), x.ctypes.data_as(_FP), i.ctypes.data_as(_IP))
    return st, n.value, x, i


def test_errors_leave_everything_unchanged(so):
    poses, scans = gr.room()
    g, r = pair(so, 0.05, max_map_points=4000, max_scan_points=1500, max_keys=3, max_keyed_points=4500, max_ref_points=64)
    for k in (5, 7):
        g.add_scan(k, scans[k]); r.add_scan(k, scans[k])
    both_insert(g, r, scans[0], poses[0])
    size = g.size()
    nan, inf = float("nan"), float("inf")
    badT = np.eye(4); badT[2, 3] = inf
    badp = scans[1].copy(); badp[77, 1] = nan
    far = scans[1][:10].copy(); far[3, 2] = 60000.0                                        # voxel index 1.2e6 at 0.05 m: found on the device
    q = scans[0][:100]
    cases = [("n = 0", lambda: g.insert(np.zeros((0, 3), F32), I4), -1),
             ("n > max_scan_points", lambda: g.insert(np.zeros((1501, 3), F32), I4), -1),
             ("add_scan: n > max_scan_points", lambda: g.add_scan(9, np.zeros((1501, 3), F32)), -1),
             ("duplicate key", lambda: g.add_scan(5, scans[2]), -1),
             ("unknown key", lambda: g.insert_key(6, I4), -1),
             ("rebuild: unknown key", lambda: g.rebuild([5, 6], [I4, I4]), -1),
             ("rebuild: keys do not ascend", lambda: g.rebuild([7, 5], [I4, I4]), -1),
             ("rebuild: a key twice", lambda: g.rebuild([5, 5], [I4, I4]), -1),
             ("rebuild: no keys", lambda: g.rebuild([], []), -1),
             ("NaN radius", lambda: g.reference(q, I4, mode="radius", radius=nan), -1),
             ("radius 0", lambda: g.reference(q, I4, mode="radius", radius=0.0), -1),
             ("NaN ref_resolution", lambda: g.reference(q, I4, mode="radius", ref_resolution=nan), -1),
             ("NaN max_dist", lambda: g.reference(q, I4, mode="knn", max_dist=nan), -1),
             ("k = 0", lambda: g.reference(q, I4, mode="knn", k=0), -1),
             ("k > 64", lambda: g.reference(q, I4, mode="knn", k=65), -1),
             ("unknown mode", lambda: g.reference(q, I4, mode=2), -1),
             ("reference: n = 0", lambda: g.reference(np.zeros((0, 3), F32), I4), -1),
             ("get_points past the end", lambda: g.points(size[0] - 1, 2), -1),
             ("non-finite point", lambda: g.insert(badp, I4), -3),
             ("non-finite T", lambda: g.insert(scans[1], badT), -3),
             ("insert_key: non-finite T", lambda: g.insert_key(5, badT), -3),
             ("add_scan: non-finite point", lambda: g.add_scan(9, badp), -3),
             ("rebuild: non-finite T", lambda: g.rebuild([5, 7], [I4, badT]), -3),
             ("reference: non-finite query", lambda: g.reference(badp, I4), -3),
             ("reference: non-finite T_out", lambda: g.reference(q, I4, T_out=badT), -3),
             ("voxel out of range", lambda: g.insert(far, I4), -1),
             ("voxel out of range by T", lambda: g.insert_key(5, gr.pose(0.0, -70000.0, 0.0, 0.1)), -1),
             ("reference voxel out of range", lambda: g.reference(q, poses[0], mode="radius", ref_resolution=1e-6), -1),
             ("n_map + n > max_map_points", lambda: [g.insert(scans[1], poses[1]), g.insert(scans[2], poses[2])], -7)]
    for name, call, status in cases:
        if name.startswith("n_map + n"):
            r.insert(scans[1], poses[1]); size = (len(r.points),) + size[1:]                # the first of the two inserts fits
        with pytest.raises(globalmap.GlobalMapError) as e:
            call()
        assert e.value.status == status, (name, e.value.status)
        assert g.size() == size, name
        same(g, r)
    # the keyed points of a rebuild exceed max_map_points: a third stored scan makes 4500 > 4000; then the store itself is full
    g.add_scan(9, scans[2]); r.add_scan(9, scans[2])
    for name, call, status in [("rebuild above max_map_points", lambda: g.rebuild([5, 7, 9], [I4, I4, I4]), -7), ("max_keys", lambda: g.add_scan(11, scans[3]), -7),
                               ("rebuild: voxel out of range", lambda: g.rebuild([5, 7], [I4, gr.pose(0.0, 0.0, 80000.0, 0.0)]), -1)]:
        with pytest.raises(globalmap.GlobalMapError) as e:
            call()
        assert e.value.status == status, (name, e.value.status)
        assert g.size() == (len(r.points), 3, 4500), name
        same(g, r)
    # n_ref > max_ref_points = 64: the count comes back, nothing is copied
    o = globalmap.default_ref_options(so, mode="radius")
    st, n, x, i = raw_reference(g, scans[0][:400], poses[0], o, 64)
    assert st == -7 and n == len(r.reference_radius(scans[0][:400], poses[0])[1]) > 64
    assert np.all(x == -7.0) and np.all(i == -7)
    # after all that the map still works: the table, the scratch table and the stored scans are as they were
    g.rebuild([5, 9], [poses[5], poses[2]]); r.rebuild([5, 9], [poses[5], poses[2]])
    same(g, r)
    x, i = g.reference(scans[5][:20], poses[5], mode="radius", radius=0.1)
    rx, ri = r.reference_radius(scans[5][:20], poses[5], 0.1, 0.3)
    assert np.array_equal(i, ri) and x.tobytes() == rx.tobytes() and 0 < len(i) <= 64
    g.close()


# ---- 6. the chain through the other rows --------------------------------------------------------------------------------------------------------------------
def test_chain_reference_align_score_posegraph_rebuild(so):
    """An 8-pose loop in the room: every scan is registered against the reference cut from the map (vgmap_reference -> vgicp_align ->
    vloop_score), goes into the map and the pose graph; the loop is closed, the graph optimised, the map rebuilt from the keyed scans at
    the poses vpgo_get_poses returns.  Checked: every reference and the rebuilt map equal the restatement fed the same poses.  No claim
    about the accuracy of the poses is made here."""
    rng = np.random.default_rng(11)
    true = [gr.pose(6.0 + 2.5 * np.cos(a), 4.0 + 1.5 * np.sin(a), 1.2, a + 1.0) for a in np.arange(8) * (2 * np.pi / 8)]
    scans = [gr.room_scan(T, 1500, seed=500 + k) for k, T in enumerate(true)]
    g, r = pair(so, 0.05)
    reg = vgicp.Vgicp(so); lv = loopverify.LoopVerify(so, max_points=1 << 14); pg = posegraph.PoseGraph(so, max_poses=16, max_factors=32)
    var = np.full(6, 1e-4)
    est = []
    for k, (Tt, s) in enumerate(zip(true, scans)):
        guess = gr.pose(*rng.normal(0, 0.02, 3), rng.normal(0, 0.005)) @ Tt
        g.add_scan(k, s); r.add_scan(k, s)
        if k:
            Tinv = np.linalg.inv(guess)
            ref, idx = g.reference(s, guess, T_out=Tinv, mode="radius")
            rx, ri = r.reference_radius(s, guess, 0.5, 0.3, Tinv)
            assert np.array_equal(idx, ri) and ref.tobytes() == rx.tobytes() and len(idx) > 200
            reg.set_target(ref, None, 0.5); reg.set_source(s)
            dT, summ = reg.align(np.eye(4))
            lv.set_target(ref); lv.set_source(s)
            score, used = lv.score(dT, max_range=1.0)
            print("scan %d: %d reference points, %d iterations, converged %d, fitness %.5f over %d" % (k, len(idx), summ.iterations, summ.converged, score, used))
            assert np.all(np.isfinite(dT))
            guess = guess @ dT
        est.append(guess)
        g.insert_key(k, guess); r.insert_key(k, guess)
        same(g, r)
        assert pg.add_pose(guess) == k
        if k == 0:
            pg.add_prior(0, guess, np.full(6, 1e-6))
        else:
            pg.add_between(k - 1, k, pg.relative(k, k - 1), var)                        # Z = T_i^-1 T_j
    closing = pg.relative(0, 7) @ gr.pose(0.03, -0.02, 0.0, 0.004)                         # the loop closure disagrees a little with the odometry
    pg.add_between(7, 0, closing, var)
    sm = pg.optimize()
    poses = pg.poses()
    print("pose graph: %d iterations, cost %.3e -> %.3e" % (sm.iterations, sm.initial_cost, sm.final_cost))
    assert np.all(np.isfinite(poses)) and not np.array_equal(poses, np.array(est))
    keys = list(range(8))
    g.rebuild(keys, poses); r.rebuild(keys, poses)
    same(g, r)
    for c in (g, reg, lv, pg):
        c.close()
