"""The restatement of include/vilcloud.h against itself and against hand-derived answers, without a GPU: the partitioned form of filter A
(what the device runs) equals the sequential loop on raw bytes, the fixtures reach every branch, and the quirks the header writes down
are the restatement's."""
import numpy as np
import pytest

import cloud_ref as ref

F = np.float32
EYE = np.eye(4, dtype=np.float32)[:3]


def raw_bytes(a):
    return np.ascontiguousarray(a).view(np.uint8)


# (kind, n, leaf, H): every kind, both table sizes of the GPU test, and the accumulation's second leaf
FIXTURES = [(k, n, leaf, H) for k in ref.KINDS for (n, leaf, H) in ((1, 0.2, 512), (700, 0.2, 64), (5000, 0.2, 512), (3000, 0.1, 512))] + [("random", 5000, 0.2, 4),
                                                                                                                                            ("lidar", 0, 0.2, 512)]


@pytest.fixture(scope="module")
def sequential():
    return {f: ref.filter_seq(ref.make_cloud(f[0], f[1]), f[2], f[3]) for f in FIXTURES}


@pytest.mark.parametrize("fix", FIXTURES, ids=lambda f: "%s-%d-%g-%d" % f)
def test_partitioned_form_equals_the_sequential_loop(sequential, fix):
    s = sequential[fix].out
    p = ref.filter_part(ref.make_cloud(fix[0], fix[1]), fix[2], fix[3])
    assert p.dtype == np.float32 and p.shape == s.shape
    assert np.array_equal(raw_bytes(p), raw_bytes(s))


def test_known_answer_six_points_four_entries():
    """leaf 1, H = 4: 7171, 3079 and 4231 are all 3 mod 4, so the bucket is 3 (ix + iy + iz) & 3.  Voxels A = (0,0,0) and B = (4,0,0) share
    bucket 0, C = (1,0,0) has bucket 3.  Order A A C B A C: B evicts A's two points, the third A evicts B, the end flushes bucket 0 (A,
    one point), then bucket 3 (C, two points)."""
    pts = F([[0.5, 0.5, 0.5, 1], [0.25, 0.75, 0.5, 3], [1.5, 0.5, 0.5, 10], [4.5, 0.25, 0.25, 5], [0.5, 0.5, 0.5, 7], [1.25, 0.5, 0.75, 20]])
    want = F([[0.375, 0.625, 0.5, 2], [4.5, 0.25, 0.25, 5], [0.5, 0.5, 0.5, 7], [1.375, 0.5, 0.625, 15]])
    ok, vox, bucket = ref.keys(pts, 1.0, 4)
    assert ok.all() and bucket.tolist() == [0, 0, 3, 0, 0, 3] and vox[3].tolist() == [4, 0, 0]
    s = ref.filter_seq(pts, 1.0, 4)
    assert (s.n_evict, s.n_nonempty, s.max_run) == (2, 2, 2)
    assert np.array_equal(raw_bytes(s.out), raw_bytes(want))
    assert np.array_equal(raw_bytes(ref.filter_part(pts, 1.0, 4)), raw_bytes(want))


def test_fixtures_reach_every_branch(sequential):
    s = sequential
    assert s[("random", 5000, 0.2, 512)].n_evict > 1000 and s[("random", 5000, 0.2, 512)].max_voxels_in_bucket > 1
    assert s[("lidar", 5000, 0.2, 512)].max_run > 1 and s[("lidar", 5000, 0.2, 512)].n_evict > 0
    one = s[("one_voxel", 5000, 0.2, 512)]
    assert (one.n_evict, one.n_nonempty, one.max_run, len(one.out)) == (0, 1, 5000, 1)                 # nothing evicts; 511 empty buckets
    alt = s[("alternating", 5000, 0.2, 512)]
    assert (alt.n_evict, alt.n_nonempty, alt.max_run, len(alt.out)) == (4999, 1, 1, 5000)             # every point evicts
    assert s[("alternating", 700, 0.2, 64)].n_evict == 699
    assert s[("lidar", 700, 0.2, 64)].n_nonempty < 64 or s[("one_voxel", 700, 0.2, 64)].n_nonempty < 64  # an empty bucket
    # negative coordinates where floor and truncation differ
    pts = ref.make_cloud("random", 5000)
    ok, vox, _ = ref.keys(pts, 0.2, 512)
    assert (vox < 0).any() and (vox != np.trunc(pts[:, :3].astype(np.float64) * 5.0)).any()
    # points on voxel faces: x * inv is an integer for some, just under one for others
    face = ref.make_cloud("faces", 5000)
    q = face[:, :3] * (F(1.0) / F(0.2))
    assert (q == np.floor(q)).sum() > 500 and (q != np.floor(q)).sum() > 500
    # dropped: NaN, +-Inf, a finite coordinate whose quotient overflows, one outside int32; a NaN intensity is carried through
    bad = ref.make_cloud("nonfinite", 5000)
    nf = s[("nonfinite", 5000, 0.2, 512)]
    ok, _, _ = ref.keys(bad, 0.2, 512)
    assert nf.n_dropped == (~ok).sum() > 400
    assert np.isnan(bad[~ok, :3]).any() and np.isinf(bad[~ok, :3]).any() and (np.abs(bad[~ok, :3]) == F(1e10)).any() and (np.abs(bad[~ok, :3]) == F(3e38)).any()
    assert np.isnan(bad[ok, 3]).any() and np.isnan(nf.out[:, 3]).any() and np.isfinite(nf.out[:, :3]).all()
    assert len(s[("lidar", 0, 0.2, 512)].out) == 0


def test_minus_zero_becomes_plus_zero():
    """step 4: the first addition of a run is 0.0f + p."""
    out = ref.filter_seq(F([[-0.0, 0.1, 0.1, -0.0]]), 0.2, 512).out
    assert raw_bytes(out[0, 0]).tolist() == [0, 0, 0, 0] and raw_bytes(out[0, 3]).tolist() == [0, 0, 0, 0]


def test_view_filter_quirks():
    assert ref.in_view(F([5, -30, 0]))                    # no lower bound: abs() is taken of a comparison
    assert not ref.in_view(F([5, 30, 0]))
    assert not ref.in_view(F([0, 0, 0])) and not ref.in_view(F([0, 1, 0])) and not ref.in_view(F([0, 0, -1]))      # x = 0: NaN or infinite quotient
    assert not ref.in_view(F([-1, 0, 0]))
    assert ref.in_view(F([25, 0, 0])) and not ref.in_view(np.nextafter(F([25, 0, 0]), F(np.inf)))
    assert ref.in_view(F([1, 10, -10])) and not ref.in_view(F([1, np.nextafter(F(10), F(np.inf)), 0]))
    assert ref.in_view(F([1, 0, -30 + 20]))               # z / x = -10
    assert not ref.in_view(F([np.nan, 0, 0])) and not ref.in_view(F([np.inf, 0, 0]))


def tiny_scan(x):
    return F([[x, 0.3, 0.1, 1.0], [x + 1.0, -0.2, 0.4, 2.0]])


def test_pop_boundary_is_strict_and_in_double():
    a = ref.Accumulator()
    a.push(100.0, EYE, tiny_scan(3.0))
    r = a.push(105.0, EYE, tiny_scan(6.0))                 # exactly 5.0 s old: stays
    assert (r.n_scans, r.n_popped, r.n_fused) == (2, 0, 4)
    b = ref.Accumulator()
    b.push(100.0, EYE, tiny_scan(3.0))
    r = b.push(float(np.nextafter(105.0, np.inf)), EYE, tiny_scan(6.0))
    assert (r.n_scans, r.n_popped, r.n_fused) == (1, 1, 2)
    # two go in one push, oldest first in the fused cloud
    c = ref.Accumulator()
    for k, t in enumerate((0.0, 1.0, 4.0)):
        c.push(t, EYE, tiny_scan(3.0 + k))
    r = c.push(6.5, EYE, tiny_scan(9.0))
    assert (r.n_scans, r.n_popped) == (2, 2) and r.fused[:, 0].tolist() == [5.0, 6.0, 9.0, 10.0]
    # a full queue is refused before anything changes
    d = ref.Accumulator(max_scans=2)
    d.push(0.0, EYE, tiny_scan(3.0)); d.push(1.0, EYE, tiny_scan(4.0))
    with pytest.raises(ref.RefError) as e:
        d.push(2.0, EYE, tiny_scan(5.0))
    assert e.value.status == -7 and len(d.queue) == 2
    assert d.push(5.5, EYE, tiny_scan(5.0)).n_popped == 1


def test_accumulation_on_the_room():
    a = ref.Accumulator()
    M, scan = ref.room_scan(0)
    r = a.push(0.0, M, scan)
    assert r.n_raw == 4800 and 1000 < r.n_scan_ds < r.n_raw and 100 < r.n_in_view < r.n_scan_ds and r.n_fused == r.n_in_view and 0 < r.n_cloud <= r.n_fused
    assert np.array_equal(raw_bytes(r.scan_ds), raw_bytes(ref.filter_part(scan, 0.2, 512)))
    assert np.array_equal(raw_bytes(r.cloud), raw_bytes(ref.filter_part(r.fused, 0.1, 512)))
    # a contracted transform would show: the fused form differs on this very scan
    kept = np.array([c for c in r.scan_ds if ref.in_view(c)], F)
    fused = ref.transform_fma(M, kept)
    assert np.array_equal(raw_bytes(ref.transform(M, kept)), raw_bytes(r.scan_world))
    differ = (raw_bytes(fused).reshape(-1, 16) != raw_bytes(r.scan_world).reshape(-1, 16)).any(axis=1)
    assert differ.sum() > 0.05 * len(kept), int(differ.sum())
    assert np.array_equal(fused[:, 3], r.scan_world[:, 3])
