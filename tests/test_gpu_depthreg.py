"""GPU parity of the LiDAR depth association (include/vildepth.h) with its float32 restatement (tests/depthreg_ref.py), through the C-ABI.

Inputs: the device's atan2f and numpy's may differ in the last bits, which can move a point across a bin edge.  Every generated cloud
therefore loses, before either side sees it, the points whose row_angle * 2 or col_angle * 2 (the restatement's values) lies within
EDGE = 1e-3 of a half-integer: 5e-4 degrees, against a float32 ulp of 1.5e-5 degrees at 180.  That is a choice of inputs, not an exclusion
of results, and it may remove at most 1 % of a cloud per viewing pose (expected 0.4 %; asserted).  With it everything downstream is
compared bit for bit: sphere cloud, neighbour indices, depths and the summary counts."""
import os
import subprocess
import tempfile

import numpy as np
import pytest

import depthreg_ref as ref
from mvil_fusion_amd import depthreg, lib
from mvil_fusion_amd.vgicp import _rot
from test_depthreg_ref import CENTRE, EYE, FILL, at, patch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EDGE = 1e-3
POSES = [(_rot(0.02, -0.03, 0.4), np.array([1.0, -2.0, 0.2])), (_rot(-0.04, 0.05, 2.3), np.array([-2.5, 1.5, 0.4])), (_rot(0.03, 0.02, -1.6), np.array([0.5, 3.0, 0.0]))]


def raw_bytes(a):
    return np.ascontiguousarray(a).view(np.uint8)


def keep_off_edges(cloud, views, edge=EDGE):
    """The input filter of the module docstring, for every (m1, m2) of `views` in turn."""
    for m1, m2 in views:
        near = ref.edge_distance(cloud, m1, m2) < edge
        assert near.sum() <= 0.01 * len(cloud), (int(near.sum()), len(cloud))
        cloud = cloud[~near]
    return cloud


def view_of(pose):
    return depthreg.view_matrices(pose[0], pose[1], *depthreg.EXTRINSIC)


def scene(seed, pose, **kw):
    cloud, feat, _ = depthreg.make_scene(pose[0], pose[1], seed=seed, **kw)
    m1, m2 = view_of(pose)
    return keep_off_edges(cloud, [(m1, m2)]), m1, m2, feat


def check(reg, m1, m2, feat, cloud, what=""):
    """`cloud` is the one resident in `reg`.  Returns the restatement's result."""
    g = reg.register(m1, m2, feat)
    sphere, nn3 = reg.debug_read()
    o = ref.register(cloud, m1, m2, feat)
    assert (g.n_cloud, g.n_in_view, g.n_sphere, g.n_with_depth) == (o.n_cloud, o.n_in_view, o.n_sphere, o.n_with_depth), what
    assert sphere.shape == o.sphere.shape and np.array_equal(raw_bytes(sphere), raw_bytes(o.sphere)), what
    assert np.array_equal(nn3, o.nn3), what
    assert np.array_equal(raw_bytes(g.depth), raw_bytes(o.depth)), what
    return o


@pytest.fixture(scope="module")
def so():
    return lib.load_vilsolve()


@pytest.fixture(scope="module")
def reg(so):
    r = depthreg.DepthReg(so, max_cloud_points=1 << 15, max_features=256)
    yield r
    r.close()


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_parity_on_the_synthetic_room(reg, seed):
    cloud, m1, m2, feat = scene(seed, POSES[seed])
    assert 15000 < len(cloud) < 25000 and len(feat) == 150
    reg.set_cloud(cloud)
    o = check(reg, m1, m2, feat, cloud, "seed %d" % seed)
    print("seed %d: cloud %d, in view %d, sphere %d, with depth %d" % (seed, o.n_cloud, o.n_in_view, o.n_sphere, o.n_with_depth))
    assert o.n_with_depth >= 30 and (o.depth == -1).sum() >= 30                     # both branches


# ---- band exactness -----------------------------------------------------------------------------------------------------------------
def direction(e_deg, a_deg):
    e, a = np.deg2rad(e_deg), np.deg2rad(a_deg)
    return np.array([np.cos(e) * np.cos(a), np.cos(e) * np.sin(a), np.sin(e)])


def band_scene():
    """64 features on an 8 x 8 grid, elevations -60 .. 60 degrees and azimuths -50 .. 50 (beyond the corners of a +-0.8 x +-0.6 image),
    each with its own cluster of cloud points.  The features of the lower four grid rows sit 2e-5 degrees under the top edge of their
    range-image row and have two close neighbours and a third one 2.50011 degrees straight above: less than the 2.500156 degrees of the
    threshold (chord 5 sin 0.5 deg), and 9e-5 degrees inside the row SIX above the feature's -- the farthest an accepted neighbour can
    be.  (Those points are 1.8e-4 bins from an edge, not 1e-3: the window between the row edge and the threshold is only 3e-4 bins wide.
    It is still 12 and more float32 ulps of their row angle, which is below 90, and 6 ulps of an atan2f result of 1 rad.)"""
    rng = np.random.default_rng(5)
    feats, pts, special = [], [], []
    for ie, e0 in enumerate(np.linspace(-60.0, 60.0, 8)):
        for a0 in np.linspace(-50.0, 50.0, 8):
            if ie < 4:
                e = (np.round((e0 + 90.0) * 2.0) * 0.5 - 90.0) + 0.25 - 2e-5
                d = direction(e, a0)
                special.append(len(feats))
                off = [(0.3, 0.1), (-0.4, -0.2), (2.50011, 0.0)]
            else:
                e = e0
                d = direction(e, a0)
                off = [(rng.uniform(-2.2, 2.2), rng.uniform(-1.0, 1.0)) for _ in range(5)]
            # feature: the view-frame direction d is sphere point p = (v.z, -v.x, -v.y)
            v = np.array([-d[1], -d[2], d[0]])
            feats.append(v / v[2])
            for de, da in off:
                pts.append(np.append(direction(e + de, a0 + da) * rng.uniform(11.5, 12.5), 1.0))
    return np.array(pts, np.float32), np.array(feats, np.float32), special


def test_band_search_is_exact_six_rows_away(reg):
    cloud, feat, special = band_scene()
    cloud = cloud[ref.edge_distance(cloud, EYE, EYE) >= 1.5e-4]
    reg.set_cloud(cloud)
    o = check(reg, EYE, EYE, feat, cloud, "band")
    frow = ref.feature_rows(feat)
    acc = o.nn3[:, 0] >= 0
    drow = np.abs(o.sphere_rc[o.nn3[acc], 0] - frow[acc, None])
    print("accepted %d of %d features; |delta row| histogram %s" % (acc.sum(), len(feat), np.bincount(drow.ravel()).tolist()))
    assert acc.sum() >= 48 and drow.max() == 6
    assert sum(bool(acc[i]) and np.abs(o.sphere_rc[o.nn3[i], 0] - frow[i]).max() == 6 for i in special) >= 16
    assert frow.min() < 70 and frow.max() > 290                                    # +-60 degrees of elevation


# ---- edge cases, each against the restatement ----------------------------------------------------------------------------------------
S9 = np.float32(2.0 ** -9)
# integer points with an exact float32 norm: 2048^2 + 64^2 + 1 = 2049^2, 3072^2 + 72^2 + 31^2 = 3073^2 (every square and sum below 2^24)
Q_A, Q_B, Q_C = np.float32([2048, 64, 1]) * S9, np.float32([2048, -64, 1]) * S9, np.float32([3072, 72, 31]) * S9           # ranges 4.001953125 (twice), 6.001953125


def tie_cloud():
    """1000 points of ONE bin: ten far ones, then 990 at exactly equal distance alternating between two different positions (squares and sums
    exact in float32: 16 + 2^-10 + 289 * 2^-18): the winner must be index 10."""
    p1, p2 = np.float32([4.0, 0.033203125, 0.03125]), np.float32([4.0, 0.03125, 0.033203125])
    rows = [np.append(2 * p1, 1.0)] * 10 + [np.append(p2 if i % 2 == 0 else p1, 1.0) for i in range(990)]
    return np.array(rows, np.float32)


def edge_cases():
    c = {}
    c["behind_the_camera"] = (np.concatenate([FILL, patch(5.0)]) * np.float32([-1, 1, 1, 1]), CENTRE)
    c["nine_bins"] = (patch(5.0), CENTRE)
    c["ten_bins"] = (np.concatenate([FILL[:1], patch(5.0)]), CENTRE)
    c["thousand_points_one_bin"] = (np.concatenate([FILL, at([180, 180, 182], [180, 182, 180], 5.0), tie_cloud()]), CENTRE)     # the tie's bin is (181, 179)
    c["x_zero"] = (np.concatenate([FILL, patch(5.0), np.float32([[0, 0, -5, 1], [0, 1, 0, 1], [0, 0, 0, 1], [0, -2, 3, 1]])]), CENTRE)
    bad = np.float32([[np.nan, 1, 1, 1], [5, np.inf, 0, 1], [5, 0, -np.inf, 1], [np.inf, np.inf, np.inf, 1], [3e38, 3e38, 0, 1], [5, 0, 0, np.nan]])
    c["nan_and_inf"] = (np.concatenate([bad[:3], FILL, bad[3:], patch(6.0)]), CENTRE)
    c["two_neighbours_in_reach"] = (np.concatenate([FILL, at([120, 121, 122], [40, 41, 42], 9.0), at([180, 180], [180, 181], 5.0)]), CENTRE)
    quad = lambda qc: np.concatenate([FILL, at(100, 106, 9.0), np.array([np.append(q, 1.0) for q in (Q_A, Q_B, qc)], np.float32)])
    c["spread_exactly_2"] = (quad(Q_C), CENTRE)
    c["spread_just_above_2"] = (quad(Q_C * np.float32(1.0 + 2.0 ** -18)), CENTRE)
    c["depth_just_below_3"] = (np.concatenate([FILL, patch(3.0 - 2e-6)]), CENTRE)
    c["depth_just_above_3"] = (np.concatenate([FILL, patch(3.0 + 2e-6)]), CENTRE)
    return c


@pytest.mark.parametrize("name", sorted(edge_cases()))
def test_edge_cases(reg, name):
    cloud, feat = edge_cases()[name]
    reg.set_cloud(cloud)
    o = check(reg, EYE, EYE, feat, cloud, name)
    rng3 = o.sphere[o.nn3[0], 3] if o.nn3[0, 0] >= 0 else None
    if name == "behind_the_camera":
        assert (o.n_in_view, o.n_sphere) == (0, 0) and o.depth[0] == -1
    if name == "nine_bins":
        assert o.n_sphere == 9 and o.depth[0] == -1
    if name == "ten_bins":
        assert o.n_sphere == 10 and o.depth[0] > 3
    if name == "thousand_points_one_bin":
        assert o.n_in_view == 9 + 1000 and o.n_sphere == 10 and o.sphere_src.tolist()[8] == 9 + 10 and 8 in o.nn3[0].tolist() and o.depth[0] > 3
    if name == "x_zero":
        assert o.n_in_view == 15                                                   # all four go: |y / x| or |z / x| is infinite, the origin has range 0
    if name == "nan_and_inf":
        assert o.n_cloud == 21 and o.n_in_view == 16 and o.depth[0] > 3            # the NaN intensity is carried along, not looked at
    if name == "two_neighbours_in_reach":
        assert o.n_sphere == 11 and o.nn3[0].tolist() == [-1, -1, -1] and o.depth[0] == -1
    if name == "spread_exactly_2":
        assert rng3.max() - rng3.min() == np.float32(2.0) and o.depth[0] > 3
    if name == "spread_just_above_2":
        assert rng3.max() - rng3.min() > np.float32(2.0) and o.depth[0] == -1
    if name == "depth_just_below_3":
        assert rng3 is not None and o.depth[0] == -1 and 2.99999 < rng3.mean() < 3.0
    if name == "depth_just_above_3":
        assert 3.0 < o.depth[0] < 3.00001


def test_no_cloud_empty_cloud_and_no_features(so, reg):
    fresh = depthreg.DepthReg(so, max_cloud_points=64, max_features=8)
    g = fresh.register(EYE, EYE, np.repeat(CENTRE, 5, axis=0))                     # no cloud set
    assert g.depth.tolist() == [-1.0] * 5 and (g.n_cloud, g.n_in_view, g.n_sphere, g.n_with_depth) == (0, 0, 0, 0)
    sphere, nn3 = fresh.debug_read()
    assert len(sphere) == 0 and nn3.tolist() == [[-1, -1, -1]] * 5
    cloud = np.concatenate([FILL, patch(5.0)])
    fresh.set_cloud(cloud)
    assert fresh.register(EYE, EYE, CENTRE).depth[0] > 3
    fresh.set_cloud(np.zeros((0, 4), np.float32))                                  # n = 0
    g = fresh.register(EYE, EYE, CENTRE)
    assert g.depth.tolist() == [-1.0] and (g.n_cloud, g.n_sphere) == (0, 0)
    fresh.set_cloud(cloud)
    g = fresh.register(EYE, EYE, np.zeros((0, 3), np.float32))                     # n_feat = 0: the cloud is still projected
    assert len(g.depth) == 0 and (g.n_cloud, g.n_in_view, g.n_sphere, g.n_with_depth) == (15, 15, 15, 0)
    sphere, _ = fresh.debug_read()
    assert np.array_equal(raw_bytes(sphere), raw_bytes(ref.register(cloud, EYE, EYE, CENTRE).sphere))
    fresh.close()


def test_sizes_beyond_the_context_are_invalid_and_write_nothing(so):
    small = depthreg.DepthReg(so, max_cloud_points=15, max_features=2)
    cloud = np.concatenate([FILL, patch(5.0)])
    small.set_cloud(cloud)
    before = small.register(EYE, EYE, CENTRE)
    with pytest.raises(depthreg.DepthRegError) as e:
        small.set_cloud(np.concatenate([cloud, cloud[:1]]))
    assert e.value.status == -1
    after = small.register(EYE, EYE, CENTRE)                                       # the resident cloud is untouched
    assert after.n_cloud == 15 and np.array_equal(raw_bytes(after.depth), raw_bytes(before.depth))
    out = np.full(8, 7.0, np.float32)
    with pytest.raises(depthreg.DepthRegError) as e:
        small.register(EYE, EYE, np.repeat(CENTRE, 3, axis=0), depth_out=out)
    assert e.value.status == -1 and out.tolist() == [7.0] * 8
    small.close()


def test_residency_leaves_no_stale_bins(reg):
    a, m1, m2, feat = scene(3, POSES[0], n_poses=2)
    b = a[::5]
    def run(cloud):
        reg.set_cloud(cloud)
        check(reg, m1, m2, feat, cloud)
        g = reg.register(m1, m2, feat); sphere, nn3 = reg.debug_read()
        return raw_bytes(g.depth).tobytes() + raw_bytes(sphere).tobytes() + raw_bytes(nn3).tobytes() + bytes([g.n_sphere & 0xff, g.n_in_view & 0xff, g.n_with_depth & 0xff])
    first, second, third = run(a), run(b), run(a)
    assert first == third and first != second


def test_ten_poses_against_one_resident_cloud(reg):
    R0, t0 = POSES[1]
    poses = [(R0 @ _rot(0.004 * k, -0.003 * k, 0.02 * k), t0 + np.array([0.05 * k, -0.03 * k, 0.01 * k])) for k in range(10)]
    cloud, feat, _ = depthreg.make_scene(R0, t0, seed=4, n_poses=2)
    views = [view_of(p) for p in poses]
    cloud = keep_off_edges(cloud, views)                                           # at most 1 % per pose
    reg.set_cloud(cloud)
    with_depth = [check(reg, m1, m2, feat, cloud, "pose %d" % k).n_with_depth for k, (m1, m2) in enumerate(views)]
    assert min(with_depth) >= 20 and len(set(with_depth)) > 1


def test_determinism(so, reg):
    cloud, m1, m2, feat = scene(5, POSES[2], n_poses=2)
    def snap(r):
        g = r.register(m1, m2, feat); sphere, nn3 = r.debug_read()
        return raw_bytes(g.depth).tobytes() + raw_bytes(sphere).tobytes() + raw_bytes(nn3).tobytes() + bytes([g.n_sphere & 0xff, g.n_in_view & 0xff, g.n_with_depth & 0xff])
    reg.set_cloud(cloud)
    a = snap(reg)
    assert snap(reg) == a and snap(reg) == a
    second = depthreg.DepthReg(so, max_cloud_points=len(cloud), max_features=len(feat))
    second.set_cloud(cloud)
    assert snap(second) == a
    second.close()


def test_profile_counts_every_kernel(reg):
    cloud, m1, m2, feat = scene(6, POSES[0], n_poses=1)
    reg.set_cloud(cloud)
    reg.profile_enable(True)
    reg.profile_read()
    for _ in range(3):
        reg.register(m1, m2, feat)
    prof = reg.profile_read()
    reg.profile_enable(False)
    assert sorted(prof) == sorted(depthreg.KERNELS) and all(n == 3 and ms > 0 for n, ms in prof.values()), prof


# ---- chain: depths -> obs8[7] -> FeatureTable -> lm_const ------------------------------------------------------------------------------
CHAIN = r'''
#include <cstdio>
#include "vilwindow_shim.hpp"
extern "C" void vil_prior_capacity(int, int*, int*, int*) {}
extern "C" int vpre_integrate(vpre_ctx*, int32_t, const int32_t*, const double*, const double*, const double*, const double*, const double*, const double*, const double*, const double*, double*, double*) { return -1; }
int main() {
    // stdin: n, then n x [x y depth]: the features of the first image and the depth channel vdepth_register gave them
    int n; if (std::scanf("%d", &n) != 1) return 1;
    std::vector<double> x(n), y(n), d(n);
    for (int i = 0; i < n; ++i) if (std::scanf("%lf %lf %lf", &x[i], &y[i], &d[i]) != 3) return 1;
    const int W = 6;
    vil::FeatureTable ft(W, 5.0, 10.0 / 460.0);
    for (int fc = 0; fc <= W; ++fc) {
        std::vector<int> ids; std::vector<double> obs;
        for (int i = 0; i < n; ++i) { ids.push_back(i); const double o[8] = {x[i] + 0.01 * fc, y[i], 1.0, 300.0 + i, 200.0, 0.1, -0.1, fc == 0 ? d[i] : -1.0}; obs.insert(obs.end(), o, o + 8); }
        ft.add_frame(fc, ids.data(), obs.data(), n, 0.0);
    }
    vil::WindowPacker pk(W + 1, ft.count()); ft.pack(pk, 240.0);
    const vil_problem* p = pk.finish();
    std::printf("%d", p->L);
    for (int l = 0; l < p->L; ++l) std::printf(" %d", (int)p->lm_const[l]);
    std::printf("\n");
    return 0;
}
'''


def test_depths_reach_lm_const_through_the_feature_table(reg):
    """The depth channel goes where the tracker puts it, obs8[7] of the feature frame (vilformat.hpp), and through vilwindow_shim.hpp's
    FeatureTable, driven as test_window_shim.py drives it: lm_const is set for exactly the features whose depth is > 0."""
    cloud, m1, m2, feat = scene(0, POSES[0])
    reg.set_cloud(cloud)
    g = reg.register(m1, m2, feat)
    assert 30 <= (g.depth > 0).sum() <= len(feat) - 30
    with tempfile.TemporaryDirectory() as d:
        src = os.path.join(d, "c.cpp"); open(src, "w").write(CHAIN)
        exe = os.path.join(d, "c")
        subprocess.check_call(["g++", "-O1", "-std=c++17", "-I", os.path.join(ROOT, "include"), src, "-o", exe])
        text = "%d\n" % len(feat) + "\n".join("%.9g %.9g %.9g" % (f[0], f[1], z) for f, z in zip(feat, g.depth))
        out = [int(v) for v in subprocess.run([exe], input=text, capture_output=True, text=True, check=True).stdout.split()]
    assert out[0] == len(feat)
    assert out[1:] == [int(z > 0) for z in g.depth]
