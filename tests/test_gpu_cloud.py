"""GPU parity of the device-resident depth cloud and filter A (include/vilcloud.h) with their restatement (tests/cloud_ref.py), through the
C-ABI.  Nothing in the contract is transcendental: every comparison is on raw bytes, no input is excluded, there is no tolerance."""
import os
import subprocess
import sys

import numpy as np
import pytest

import cloud_ref as ref
from mvil_fusion_amd import cloud, depthreg, lib

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
WG = cloud.WG_POINTS
SIZES = (0, 1, 63, 64, 65, WG - 1, WG, WG + 1, 5000, 2 * WG + 1)         # wave edges, one workgroup's range +- 1, two ranges + 1
# stamps of the chain: scan 5 arrives when scan 0 is exactly 5.0 s old (it stays), scan 6 pops scans 0 and 1 in one push, 8 and 9 pop one each
STAMPS = (10.0, 10.5, 13.0, 13.5, 14.0, 15.0, 15.75, 16.0, 18.25, 18.75)


def raw_bytes(a):
    return np.ascontiguousarray(a).view(np.uint8)


def same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(raw_bytes(a), raw_bytes(b))


@pytest.fixture(scope="module")
def so():
    return lib.load_vilsolve()


@pytest.fixture(scope="module")
def dc(so):
    d = cloud.DepthCloud(so, max_scan_points=4800, max_scans=6)
    yield d
    d.close()


@pytest.fixture(scope="module")
def chain():
    """The restatement's ten pushes, computed once: [(stamp, matrix, scan, Pushed)]."""
    acc = ref.Accumulator(max_scan_points=4800, max_scans=6)
    out = []
    for k, t in enumerate(STAMPS):
        M, scan = ref.room_scan(k)
        out.append((t, M, scan, acc.push(t, M, scan)))
    return out


@pytest.mark.parametrize("hist", [512, 64])
@pytest.mark.parametrize("kind", ref.KINDS)
def test_filter_against_the_restatement(dc, kind, hist):
    for n in SIZES:
        pts = ref.make_cloud(kind, n)
        want = ref.filter_seq(pts, ref.LEAF, hist)
        got = dc.filter(pts, ref.LEAF, hist)
        assert got.shape == want.out.shape, (kind, hist, n, got.shape, want.out.shape)
        assert same(got, want.out), (kind, hist, n)
        if kind == "alternating":
            assert len(got) == n                                                 # every point evicts
        if kind == "one_voxel":
            assert len(got) == min(n, 1)                                         # one run, one thread's sum
        if kind == "nonfinite" and n >= 5000:
            assert want.n_dropped > 400


def test_filter_other_table_sizes_and_refusals(dc):
    pts = ref.make_cloud("random", 3000)
    for hist in (1, 2, cloud.MAX_HIST):
        assert same(dc.filter(pts, 0.1, hist), ref.filter_seq(pts, 0.1, hist).out), hist
    for leaf, hist in ((0.0, 512), (-0.2, 512), (float("nan"), 512), (float("inf"), 512), (0.2, 0), (0.2, 96), (0.2, 2 * cloud.MAX_HIST)):
        with pytest.raises(cloud.CloudError) as e:
            dc.filter(pts, leaf, hist)
        assert e.value.status == cloud.ERR_INVALID_ARGUMENT, (leaf, hist)
    with pytest.raises(cloud.CloudError) as e:
        dc.filter(np.zeros((4800 * 6 + 1, 4), F), 0.2)
    assert e.value.status == cloud.ERR_INVALID_ARGUMENT


def check_push(d, r, s, what):
    assert cloud.counts(s) == (r.n_raw, r.n_scan_ds, r.n_in_view, r.n_scans, r.n_popped, r.n_fused, r.n_cloud), what
    assert same(d.debug_read(cloud.DBG_SCAN_DS), r.scan_ds), what
    assert same(d.debug_read(cloud.DBG_SCAN_WORLD), r.scan_world), what
    assert same(d.debug_read(cloud.DBG_FUSED), r.fused), what
    got = d.read_cloud()
    assert len(got) == s.n_cloud and same(got, r.cloud), what


def test_chain_of_ten_scans(dc, chain):
    dc.reset()
    assert len(dc.read_cloud()) == 0 and len(dc.debug_read(cloud.DBG_FUSED)) == 0
    for k, (t, M, scan, r) in enumerate(chain):
        check_push(dc, r, dc.push_scan(t, M, scan), "scan %d" % k)
    pops = [r.n_popped for _, _, _, r in chain]
    assert pops[5] == 0 and chain[5][3].n_scans == 6 and pops[6] == 2 and sum(pops) == 4, pops
    assert all(r.n_in_view > 100 and r.n_cloud > 100 for _, _, _, r in chain)
    # a filter call in between touches neither the queue nor the stages
    dc.filter(ref.make_cloud("random", 5000), 0.2)
    assert same(dc.read_cloud(), chain[-1][3].cloud) and same(dc.debug_read(cloud.DBG_FUSED), chain[-1][3].fused)


def test_options_are_honoured(so):
    d = cloud.DepthCloud(so, max_scan_points=4800, max_scans=3)
    kw = dict(leaf_scan=0.3, leaf_cloud=0.15, hist_size=64, max_coord=8.0, max_ratio=2.0, window_s=1.0)
    acc = ref.Accumulator(max_scan_points=4800, max_scans=3, **kw)
    opts = cloud.default_options(so, **kw)
    for k, t in enumerate((0.0, 1.0, 2.5)):
        M, scan = ref.room_scan(k)
        check_push(d, acc.push(t, M, scan), d.push_scan(t, M, scan, opts), "scan %d" % k)
    d.close()


def test_hand_over_to_the_depth_association(so, dc, chain):
    dc.reset()
    for t, M, scan, _ in chain[:3]:
        s = dc.push_scan(t, M, scan)
    world = chain[2][3].cloud
    assert s.n_cloud == len(world) > 1000
    # the viewing pose: the third scan's; features on the image plane
    M = chain[2][1].astype(np.float64)
    m1, m2 = depthreg.view_matrices(M[:, :3], M[:, 3], *depthreg.EXTRINSIC)
    rng = np.random.default_rng(3)
    feat = np.concatenate([rng.uniform(-0.6, 0.6, (120, 1)), rng.uniform(-0.45, 0.45, (120, 1)), np.ones((120, 1))], axis=1).astype(F)
    a = depthreg.DepthReg(so, max_cloud_points=len(world), max_features=128)
    b = depthreg.DepthReg(so, max_cloud_points=len(world), max_features=128)

    def snap(reg):
        g = reg.register(m1, m2, feat); sphere, nn3 = reg.debug_read()
        return (g.n_cloud, g.n_in_view, g.n_sphere, g.n_with_depth), raw_bytes(g.depth).tobytes(), raw_bytes(sphere).tobytes(), raw_bytes(nn3).tobytes()
    dc.publish(a)
    b.set_cloud(world)
    sa, sb = snap(a), snap(b)
    assert sa == sb
    assert sa[0][0] == len(world) and sa[0][2] >= depthreg.MIN_SPHERE and 0 < sa[0][3] < len(feat), sa[0]
    # too small a depth context: refused, its cloud and results stay
    small = depthreg.DepthReg(so, max_cloud_points=len(world) - 1, max_features=128)
    small.set_cloud(world[::2])
    before = snap(small)
    with pytest.raises(cloud.CloudError) as e:
        dc.publish(small)
    assert e.value.status == cloud.ERR_CAPACITY
    assert snap(small) == before and before[0][0] == len(world[::2])
    # no cloud: the "no cloud" state of vdepth_set_cloud(0)
    dc.reset()
    dc.publish(a)
    assert a.register(m1, m2, feat).n_cloud == 0
    for r in (a, b, small):
        r.close()


def test_errors_leave_the_state_alone(so):
    d = cloud.DepthCloud(so, max_scan_points=4800, max_scans=3)
    acc = ref.Accumulator(max_scan_points=4800, max_scans=3)
    seq = [(0.0, 0), (1.0, 1), (2.0, 2)]
    for t, k in seq:
        M, scan = ref.room_scan(k)
        check_push(d, acc.push(t, M, scan), d.push_scan(t, M, scan), "scan %d" % k)
    M, scan = ref.room_scan(3)
    bad_M = M.copy(); bad_M[1, 2] = np.inf
    refused = [(3.0, M, scan, cloud.ERR_CAPACITY),                                              # three scans would still be live
               (6.5, M, np.concatenate([scan, scan[:1]]), cloud.ERR_INVALID_ARGUMENT),         # n > max_scan_points
               (6.5, bad_M, scan, cloud.ERR_INVALID_ARGUMENT), (float("nan"), M, scan, cloud.ERR_INVALID_ARGUMENT)]
    before = (raw_bytes(d.read_cloud()).tobytes(), raw_bytes(d.debug_read(cloud.DBG_FUSED)).tobytes())
    for t, m, s, status in refused:
        with pytest.raises(cloud.CloudError) as e:
            d.push_scan(t, m, s)
        assert e.value.status == status, (t, status)
        with pytest.raises(ref.RefError) as e2:
            acc.push(t, m, s)
        assert e2.value.status == status
    assert (raw_bytes(d.read_cloud()).tobytes(), raw_bytes(d.debug_read(cloud.DBG_FUSED)).tobytes()) == before
    r = acc.push(6.5, M, scan)                                                                  # pops two; what the restatement gives without the refused calls
    assert r.n_popped == 2
    check_push(d, r, d.push_scan(6.5, M, scan), "after the refusals")
    # reset and replay reproduce the first run
    first = raw_bytes(d.read_cloud()).tobytes()
    d.reset(); acc.reset()
    assert len(d.read_cloud()) == 0
    for t, k in seq + [(6.5, 3)]:
        M, scan = ref.room_scan(k)
        check_push(d, acc.push(t, M, scan), d.push_scan(t, M, scan), "replay %d" % k)
    assert raw_bytes(d.read_cloud()).tobytes() == first
    d.close()


CHILD = r"""
import sys
sys.path.insert(0, %r); sys.path.insert(0, %r)
import __graft_entry__ as graft
graft.load_package()
import hashlib
import numpy as np
import cloud_ref as ref
from mvil_fusion_amd import cloud, lib
d = cloud.DepthCloud(lib.load_vilsolve(), max_scan_points=4800, max_scans=6)
h = hashlib.sha256()
for k, t in enumerate(%r):
    M, scan = ref.room_scan(k)
    s = d.push_scan(t, M, scan)
    h.update(repr(cloud.counts(s)).encode()); h.update(d.read_cloud().tobytes()); h.update(d.debug_read(cloud.DBG_FUSED).tobytes())
h.update(d.filter(ref.make_cloud("random", 5000), 0.2).tobytes())
d.close()
print("digest", h.hexdigest())
"""


def test_reproducible_across_contexts_and_processes(so, dc, chain):
    import hashlib
    n = 5

    def run(d):
        d.reset()
        h = hashlib.sha256()
        for t, M, scan, _ in chain[:n]:
            s = d.push_scan(t, M, scan)
            h.update(repr(cloud.counts(s)).encode()); h.update(d.read_cloud().tobytes()); h.update(d.debug_read(cloud.DBG_FUSED).tobytes())
        h.update(d.filter(ref.make_cloud("random", 5000), 0.2).tobytes())
        return h.hexdigest()
    a = run(dc)
    assert run(dc) == a
    other = cloud.DepthCloud(so, max_scan_points=5000, max_scans=9)                 # another context, other capacities
    assert run(other) == a
    other.close()
    code = CHILD % (ROOT, os.path.join(ROOT, "tests"), STAMPS[:n])
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=120)      # a fresh child process, never an exec
    assert out.returncode == 0, out.stderr[-2000:]
    assert out.stdout.split()[-2:] == ["digest", a]


def test_profile_counts_every_kernel(dc, chain):
    dc.reset()
    dc.profile_enable(True)
    dc.profile_read()
    for t, M, scan, _ in chain[:2]:
        dc.push_scan(t, M, scan)
    prof = dc.profile_read()
    dc.profile_enable(False)
    assert sorted(prof) == sorted(cloud.KERNELS)
    per_push = {k: 2 for k in cloud.KERNELS}                                         # filter A runs twice per push
    per_push.update(k_cloud_scan=5, k_cloud_view=1, k_cloud_place=1, k_cloud_fuse=1)
    assert {k: n for k, (n, _) in prof.items()} == {k: 2 * v for k, v in per_push.items()}, prof
    assert all(ms > 0 for _, ms in prof.values()), prof
    assert all(n == 0 for n, _ in dc.profile_read().values())
