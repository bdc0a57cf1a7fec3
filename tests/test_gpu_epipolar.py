"""include/vilepi.h on the GPU against tests/epipolar_ref.py.  The lift, the virtual-camera points, the undistorted points and the velocities
are compared on raw bits (unfused fp64 in a fixed order, no transcendental).  Of the RANSAC every integer is compared for equality: the
sample of every consumed hypothesis, its count, the winner, the consumed count and the status.  That is valid only where no decision sits on
a rounding boundary, so each such test first asserts on the restatement alone that the margin min |err / thr^2 - 1| over everything
evaluated is at least 1e-7, and prints the device's.  The winner's F is compared at unit norm and fixed sign under a cap of 1e-10 and then,
since the measured difference was zero in every case, on its raw bits."""
import hashlib
import os
import subprocess
import sys

import numpy as np
import pytest

import epipolar_ref as er
from mvil_fusion_amd import epipolar, lib, track
from test_epipolar_ref import CASES, NOISY8_SEED, SCENE_SEED, solved

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
F32 = np.float32
VIRTUAL = dict(er.VIRTUAL, focal=460.0, width=640, height=480)
REF_CAM = er.Camera(**er.REFERENCE_CAMERA)


@pytest.fixture(scope="module")
def so():
    return lib.load_vilsolve()


@pytest.fixture(scope="module")
def ep(so):
    """the context most tests share: the scenes' camera, the reference's max_iters"""
    e = epipolar.Epipolar(so, VIRTUAL, max_points=4096, max_iters=1000)
    yield e
    e.close()


def same(a, b, what):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.dtype == b.dtype and a.shape == b.shape, (what, a.dtype, b.dtype, a.shape, b.shape)
    if a.tobytes() != b.tobytes():
        bad = np.flatnonzero((a.view(np.uint8).reshape(len(a), -1) != b.view(np.uint8).reshape(len(b), -1)).any(axis=1)) if a.ndim and len(a) else []
        raise AssertionError("%s differs in %d rows, first %s: device %s, restatement %s" % (what, len(bad), bad[:5], a[bad[:3]] if len(bad) else a, b[bad[:3]] if len(bad) else b))


def against(e, cur, forw, r, what, thr=1.0, confidence=0.99, seed=1):
    """one vepi_reject against the restatement's Result r"""
    assert r.margin >= 1e-7, "%s: a decision of the restatement sits on a rounding boundary (margin %.3g): change the scene's seed" % (what, r.margin)
    st, s = e.reject(cur, forw, thr, confidence, seed)
    p1, p2 = e.debug_points()
    same(p1, r.p1, what + ": virtual points of cur"); same(p2, r.p2, what + ": virtual points of forw")
    samples, counts, margins = e.debug_hypotheses()
    assert s.evaluated >= s.consumed == r.consumed, (what, s.evaluated, s.consumed, r.consumed)
    same(samples[:r.consumed], r.samples, what + ": samples"); same(counts[:r.consumed], r.counts, what + ": counts")
    assert (s.found, s.best_hypothesis, s.n_inliers, s.n_points) == (r.found, r.best_hypothesis, r.n_inliers if r.found else len(cur), len(cur)), what
    same(st, r.status, what + ": status")
    dF = 0.0
    if r.found:
        dF = float(np.abs(er.unit_F(e.debug_F()) - er.unit_F(r.F)).max())
        assert dF <= 1e-10, (what, dF)                      # the cap: a slip in the normalisation or the rank-2 step moves it by O(1)
        same(e.debug_F(), r.F, what + ": F")                # measured: zero in every test here (fp64 sqrt and division round correctly on both sides), so equality
    print("%s: consumed %d, evaluated %d in %d launches, margin device %.3g restatement %.3g, |dF| %.3g" %
          (what, s.consumed, s.evaluated, s.launches, margins[:r.consumed].min(), r.margin, dF))
    return st, s, dF


# ---- lift and undistort --------------------------------------------------------------------------------------------------------------
def undistort_calls(n, seed=0):
    """three calls' (xy, ids, dt): ids -1, duplicated ids (the first occurrence counts), ids absent from the call before, reordered ids"""
    rng = np.random.default_rng(seed + n)
    xy0 = np.stack([rng.uniform(0, 639, n), rng.uniform(0, 479, n)], axis=1).astype(F32)
    ids0 = (100 + np.arange(n)).astype(np.int32)
    ids0[::5] = -1
    if n > 3:
        ids0[n // 2] = ids0[1]; ids0[n - 1] = ids0[1]                                   # one id three times
    perm = rng.permutation(n)
    xy1 = (xy0[perm] + rng.uniform(-2, 2, (n, 2))).astype(F32)
    ids1 = ids0[perm].copy()
    ids1[rng.permutation(n)[:max(1, n // 7)]] = 5000 + np.arange(max(1, n // 7))        # new ids
    xy2 = (xy1[::-1] + rng.uniform(-2, 2, (n, 2))).astype(F32)
    ids2 = ids1[::-1].copy()
    return (xy0, ids0, 0.05), (xy1, ids1, 0.04), (xy2, ids2, 0.0625)


@pytest.mark.parametrize("n", (1, 63, 64, 65, 4096))
def test_undistort_chain_equals_the_restatement_bit_for_bit(so, n):
    e = epipolar.Epipolar(so, epipolar.REFERENCE_CAMERA, max_points=max(8, n), max_iters=4)
    ref = er.Undistorter(REF_CAM)
    moved = 0
    for k, (xy, ids, dt) in enumerate(undistort_calls(n)):
        un, vel = e.undistort(xy, ids, dt)
        r_un, r_vel = ref.undistort(xy, ids, dt)
        same(un, r_un, "un_xy of call %d" % k); same(vel, r_vel, "vel_xy of call %d" % k)
        assert k or not vel.any()
        moved += int(vel.any(axis=1).sum())
    assert moved > 0 or n == 1
    if n >= 8:                                              # the same lift through vepi_reject's debug hook
        (a, _, _), (b, _, _), _ = undistort_calls(n)
        e.reject(a, b)
        p1, p2 = e.debug_points()
        same(p1, REF_CAM.virtual(a), "virtual points of cur"); same(p2, REF_CAM.virtual(b), "virtual points of forw")
    e.reset()                                               # after the reset: zero velocities, the table starts again
    xy, ids, dt = undistort_calls(n)[1]
    un, vel = e.undistort(xy, ids, dt)
    ref.reset()
    same(un, ref.undistort(xy, ids, dt)[0], "un_xy after the reset")
    assert not vel.any()
    un, vel = e.undistort(xy, ids, 0.0)                     # dt = 0: 0 / 0 where a point met itself; NaN payloads are not compared
    r_un, r_vel = ref.undistort(xy, ids, 0.0)
    assert np.array_equal(vel, r_vel, equal_nan=True) and (n == 1 or np.isnan(vel).any())
    un0, vel0 = e.undistort(np.zeros((0, 2), F32), np.zeros(0, np.int32), 0.05)          # n = 0 empties the table
    assert len(un0) == 0
    assert not e.undistort(xy, ids, 0.05)[1].any()
    e.close()


# ---- reject --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("noise", (0.0, 0.05))
@pytest.mark.parametrize("n,n_out", CASES)
def test_reject_equals_the_restatement(ep, n, n_out, noise):
    cur, forw, labels, _, r = solved(n, n_out, noise)
    st, s, _ = against(ep, cur, forw, r, "n %d, %d outliers, noise %g" % (n, n_out, noise))
    if noise == 0.0:
        same(st, labels, "status against the planted labels")


@pytest.mark.parametrize("n,n_out", ((150, 60), (12, 3)))
def test_result_does_not_depend_on_batch_or_read_back(so, n, n_out):
    cur, forw, _, _, r = solved(n, n_out)
    outs = []
    for batch, readback in ((1, 0), (7, 0), (64, 0), (1000, 0), (1, 1), (64, 1), (1000, 1)):
        e = epipolar.Epipolar(so, VIRTUAL, max_points=256, max_iters=1000, batch=batch, readback=readback)
        st, s, _ = against(e, cur, forw, r, "batch %d read-back %d" % (batch, readback))
        assert s.launches == -(-s.evaluated // batch) and s.evaluated <= -(-r.consumed // batch) * batch
        outs.append((st.tobytes(), s.found, s.best_hypothesis, s.n_inliers, s.consumed, e.debug_F().tobytes()))
        e.close()
    assert all(o == outs[0] for o in outs)


def test_fewer_than_eight_points_launch_nothing(so):
    e = epipolar.Epipolar(so, VIRTUAL, max_points=64, max_iters=100)
    e.profile_enable(True); e.profile_read()
    cur, forw, _, _ = er.scene(7, 0, 0.0, SCENE_SEED)
    st, s = e.reject(cur, forw)
    assert st.tolist() == [1] * 7 and (s.launches, s.evaluated, s.consumed, s.found, s.best_hypothesis, s.n_inliers) == (0, 0, 0, 0, -1, 7)
    assert all(v == (0, 0.0) for v in e.profile_read().values())
    st, s = e.reject(np.zeros((0, 2), F32), np.zeros((0, 2), F32))
    assert len(st) == 0 and s.launches == 0
    c, f, _, _, r = solved(12, 3)
    e.reject(c, f)
    p = e.profile_read()
    assert p["k_epi_lift"][0] == 1 and p["k_epi_hyp"][0] == 1 and p["k_epi_hyp"][1] > 0 and p["k_epi_undist"][0] == 0
    e.undistort(c, np.arange(12), 0.05)
    assert e.profile_read()["k_epi_undist"][0] == 1
    e.close()


def test_no_model_with_eight_inliers_keeps_every_point(ep):
    cur, forw, _, _ = er.scene(8, 0, 0.2, NOISY8_SEED)
    r = er.reject(er.Camera(**er.VIRTUAL), cur, forw)
    assert r.found == 0 and r.consumed == 1000
    st, s, _ = against(ep, cur, forw, r, "n 8, noise 0.2")
    assert st.tolist() == [1] * 8 and (s.found, s.best_hypothesis, s.consumed) == (0, -1, 1000)
    with pytest.raises(epipolar.EpipolarError) as e:        # there is no winner's F to read
        ep.debug_F()
    assert e.value.status == -1


def test_4096_points_with_a_fifth_outliers(ep):
    cur, forw, labels, _ = er.scene(4096, 819, 0.0, SCENE_SEED)
    r = er.reject(er.Camera(**er.VIRTUAL), cur, forw)
    assert r.found == 1 and np.array_equal(r.status, labels)
    st, s, _ = against(ep, cur, forw, r, "n 4096, 819 outliers")
    assert int(st.sum()) == 4096 - 819 == s.n_inliers


def test_errors_write_nothing_and_a_later_call_is_unaffected(so):
    import ctypes as C
    e = epipolar.Epipolar(so, VIRTUAL, max_points=64, max_iters=1000)
    cur, forw, _, _, r = solved(63, 12)
    c65, f65, _, _ = er.scene(65, 13, 0.0, SCENE_SEED)
    guard = np.full(80, 9, np.uint8)
    for args in ((c65, f65, 1.0, 0.99), (cur, forw, 0.0, 0.99), (cur, forw, -1.0, 0.99), (cur, forw, float("nan"), 0.99), (cur, forw, float("inf"), 0.99),
                 (cur, forw, 1.0, 0.0), (cur, forw, 1.0, 1.0), (cur, forw, 1.0, float("nan"))):
        with pytest.raises(epipolar.EpipolarError) as err:
            e.reject(*args, status_out=guard)
        assert err.value.status == -1 and (guard == 9).all(), args[2:]
    f = so.vepi_reject; f.restype = C.c_int
    p = lambda a: C.c_void_p(a.ctypes.data)
    for ptrs in ((None, p(forw), p(guard)), (p(cur), None, p(guard)), (p(cur), p(forw), None)):
        assert f(e.ctx, C.c_int32(63), ptrs[0], ptrs[1], C.c_double(1.0), C.c_double(0.99), C.c_uint64(1), ptrs[2], None) == -1
    assert f(e.ctx, C.c_int32(-1), p(cur), p(forw), C.c_double(1.0), C.c_double(0.99), C.c_uint64(1), p(guard), None) == -1
    assert (guard == 9).all()
    with pytest.raises(epipolar.EpipolarError) as err:      # nothing was launched yet: nothing to read
        e.debug_points()
    assert err.value.status == -1
    against(e, cur, forw, r, "after the errors")
    # vepi_undistort: an error keeps the table
    xy, ids, dt = undistort_calls(63)[0]
    ref = er.Undistorter(er.Camera(**er.VIRTUAL))
    e.undistort(xy, ids, dt); ref.undistort(xy, ids, dt)
    un_g = np.full((80, 2), 7.0, F32); vel_g = np.full((80, 2), 7.0, F32)
    with pytest.raises(epipolar.EpipolarError) as err:
        e.undistort(c65, np.arange(65), 0.05, un_out=un_g, vel_out=vel_g)
    assert err.value.status == -1 and (un_g == 7.0).all() and (vel_g == 7.0).all()
    g = so.vepi_undistort; g.restype = C.c_int
    assert g(e.ctx, C.c_int32(63), p(xy), None, C.c_double(0.05), p(un_g), p(vel_g)) == -1 and (un_g == 7.0).all()
    xy1, ids1, dt1 = undistort_calls(63)[1]
    un, vel = e.undistort(xy1, ids1, dt1)
    r_un, r_vel = ref.undistort(xy1, ids1, dt1)
    same(un, r_un, "un_xy after the errors"); same(vel, r_vel, "vel_xy after the errors")
    assert vel.any()
    e.close()


# ---- reproducibility -------------------------------------------------------------------------------------------------------------------
def run_chain(so):
    """three rejects and an undistort chain; the digest of every output, F's bits included"""
    h = hashlib.sha256()
    e = epipolar.Epipolar(so, epipolar.REFERENCE_CAMERA, max_points=256, max_iters=1000, batch=64)
    for n, n_out, noise in ((150, 60, 0.05), (65, 13, 0.0), (12, 3, 0.05)):
        cur, forw, _, _ = er.scene(n, n_out, noise, SCENE_SEED)
        st, s = e.reject(cur, forw, 1.0, 0.99, 7)
        samples, counts, margins = e.debug_hypotheses()
        for a in (st, samples, counts, margins, e.debug_F() if s.found else st, *e.debug_points()):
            h.update(np.ascontiguousarray(a).tobytes())
        h.update(repr((s.found, s.best_hypothesis, s.n_inliers, s.consumed, s.evaluated)).encode())
    for xy, ids, dt in undistort_calls(200):
        for a in e.undistort(xy, ids, dt):
            h.update(a.tobytes())
    e.close()
    return h.hexdigest()


def test_bit_reproducible_across_runs_and_processes(so):
    a = run_chain(so)
    assert run_chain(so) == a
    out = subprocess.run([sys.executable, os.path.join(HERE, "epipolar_child.py")], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr[-2000:]
    child = [l for l in out.stdout.splitlines() if l.startswith("digest ")]
    assert child == ["digest " + a], (child, a)


# ---- track -> reject -> undistort ------------------------------------------------------------------------------------------------------
def parallax_pair(height, width, seed=2):
    """Two images of the texture of track.py as a camera moving sideways sees two depths: the upper half of the second image is the texture
    moved by (1, 0) px, the lower half by (9, 0) px.  All flow is along x, in two magnitudes, so F is unique (up to scale [[0, 0, 0], [0, 0, -1],
    [0, 1, 0]]: the epipolar lines are the image rows) -- unlike one drift of the whole image, see test_chain_on_the_drifting_sequence."""
    tex = track.Texture(height, width, seed)
    second = tex.render((1.0, 0.0))
    second[height // 2:] = tex.render((9.0, 0.0))[height // 2:]
    return tex.render((0.0, 0.0)), second


def moved_fifth(forw, k=1):
    """every fifth point moved by 10 px, 45 - 135 degrees off the x axis to either side: at least 7 px across the rows"""
    moved = np.zeros(len(forw), bool); moved[k::5] = True
    m = int(moved.sum())
    ang = np.deg2rad(45.0 + 90.0 * ((np.arange(m) * 7) % m) / max(m - 1, 1)) * np.where(np.arange(m) % 2, 1.0, -1.0)
    out = forw.copy(); out[moved] += (10.0 * np.stack([np.cos(ang), np.sin(ang)], axis=1)).astype(F32)
    return out, moved


CHAIN_CAM = dict(fx=300.0, fy=300.0, cx=128.0, cy=96.0, k1=0.0, k2=0.0, p1=0.0, p2=0.0, focal=460.0, width=256, height=192)


def test_chain_from_tracked_points(so):
    """vtrack_detect and vtrack_track on a pair with parallax, a fifth of the tracked points moved by 10 px, vepi_reject, vepi_undistort of
    what vepi_reject kept: the moved points go, the rest stay, and every output equals the restatement's.  The camera has no distortion, so
    that the synthetic images are exact images of a rigid scene; points whose LK window straddles the seam between the halves are left out."""
    H, W = CHAIN_CAM["height"], CHAIN_CAM["width"]
    rcam = er.Camera(**CHAIN_CAM)
    first, second = parallax_pair(H, W)
    t = track.Tracker(so, W, H, max_level=2, max_points=256, max_candidates=H * W)
    e = epipolar.Epipolar(so, CHAIN_CAM, max_points=256, max_iters=1000)
    ref = er.Undistorter(rcam)
    t.push_image(first)
    _, pts, _ = t.detect(np.zeros((0, 2), F32), 12, 150, 0.01)
    pts = pts[(np.abs(pts[:, 1] - H / 2) > 24) & (pts[:, 0] >= 16) & (pts[:, 0] < W - 30) & (pts[:, 1] >= 16) & (pts[:, 1] < H - 16)]      # LK windows inside one half of both images
    ids = np.arange(len(pts), dtype=np.int32)
    un, vel = e.undistort(pts, ids, 0.05)
    r_un, _ = ref.undistort(pts, ids, 0.05)
    same(un, r_un, "un_xy of the first image"); assert not vel.any()
    t.push_image(second)
    forw, st, _ = t.track(pts)
    cur, forw, ids = pts[st == 1], forw[st == 1], ids[st == 1]
    upper = cur[:, 1] < H / 2
    flow = forw - cur
    assert upper.sum() >= 15 and (~upper).sum() >= 15
    assert np.abs(flow[upper] - [1.0, 0.0]).max() < 0.2 and np.abs(flow[~upper] - [9.0, 0.0]).max() < 0.2      # the tracker follows both depths
    forw, moved = moved_fifth(forw)
    r = er.reject(rcam, cur, forw)
    status, s, _ = against(e, cur, forw, r, "parallax pair, %d points" % len(cur))
    print("%d of %d moved points kept, %d of %d others dropped" % (int(status[moved].sum()), int(moved.sum()), int((1 - status[~moved]).sum()), int((~moved).sum())))
    assert moved.sum() >= 8 and not status[moved].any(), "a moved point stayed"
    assert status[~moved].all(), "an unmoved point went"
    assert s.found == 1 and s.n_inliers == int((~moved).sum())
    pts, ids = forw[status == 1], ids[status == 1]          # the caller's reduceVector on the status alone
    un, vel = e.undistort(pts, ids, 0.05)
    r_un, r_vel = ref.undistort(pts, ids, 0.05)
    same(un, r_un, "un_xy of the second image"); same(vel, r_vel, "vel_xy of the second image")
    px = vel * 0.05 * CHAIN_CAM["fx"]                       # the flow again, in px per image
    assert np.abs(px[pts[:, 1] < H / 2] - [1.0, 0.0]).max() < 0.2 and np.abs(px[pts[:, 1] >= H / 2] - [9.0, 0.0]).max() < 0.2
    t.close(); e.close()


def test_chain_on_the_drifting_sequence(so):
    """The same chain on the synthetic sequence of track.py, where the whole texture drifts by one vector t.  For such a field every
    F = [[0, 0, a1], [0, 0, a2], [-a1, -a2, c]] with a . t + c = 0 is exact: x2^T F x1 = a . (x2 - x1) + c, a line through t in the plane of
    displacements, in ANY direction a.  A sample that holds one moved point turns that line through the moved point's displacement and
    counts an inlier more than a clean sample does, so the count-maximal hypothesis keeps moved points by construction and "the moved
    points go, the rest stay" cannot be asserted here; test_chain_from_tracked_points asserts it where there is parallax.  This test runs the
    chain twice over a camera with distortion and the resident id table: the device equals the restatement throughout, the chain goes on with
    what vepi_reject kept, and the velocities are the flow again.  How many moved points stayed is printed, not asserted."""
    H, W = 192, 256
    cam = dict(fx=300.0, fy=300.0, cx=128.0, cy=96.0, k1=-0.05, k2=0.01, p1=0.0, p2=0.0, focal=460.0, width=W, height=H)
    rcam = er.Camera(**cam)
    images, shifts = track.sequence(H, W, 3, seed=2)
    t = track.Tracker(so, W, H, max_level=2, max_points=256, max_candidates=H * W)
    e = epipolar.Epipolar(so, cam, max_points=256, max_iters=1000)
    ref = er.Undistorter(rcam)
    t.push_image(images[0])
    _, pts, _ = t.detect(np.zeros((0, 2), F32), 12, 120, 0.01)
    ids = np.arange(len(pts), dtype=np.int32)
    assert len(pts) >= 60
    un, vel = e.undistort(pts, ids, 0.05)
    r_un, r_vel = ref.undistort(pts, ids, 0.05)
    same(un, r_un, "un_xy of the first image"); assert not vel.any()
    for k in (1, 2):
        t.push_image(images[k])
        forw, st, _ = t.track(pts)
        cur, forw, ids = pts[st == 1], forw[st == 1], ids[st == 1]
        flow = np.median(forw - cur, axis=0)
        assert np.abs(flow - (np.array(shifts[k]) - np.array(shifts[k - 1]))).max() < 0.1
        moved = np.zeros(len(cur), bool); moved[k::5] = True
        m = int(moved.sum())
        ang = np.deg2rad((np.arange(m) * 7 % m) * (180.0 / m) + 180.0 * (np.arange(m) % 2))          # every direction once
        forw = forw.copy(); forw[moved] += (10.0 * np.stack([np.cos(ang), np.sin(ang)], axis=1)).astype(F32)
        r = er.reject(rcam, cur, forw)
        status, s, _ = against(e, cur, forw, r, "image %d, %d points" % (k, len(cur)))
        kept_moved, lost_others = int(status[moved].sum()), int((1 - status[~moved]).sum())
        print("image %d: %d of %d moved points kept, %d of %d others dropped" % (k, kept_moved, m, lost_others, len(cur) - m))
        assert s.found == 1 and s.n_inliers == int(status.sum()) >= 8
        pts, ids = forw[status == 1], ids[status == 1]
        un, vel = e.undistort(pts, ids, 0.05)
        r_un, r_vel = ref.undistort(pts, ids, 0.05)
        same(un, r_un, "un_xy of image %d" % k); same(vel, r_vel, "vel_xy of image %d" % k)
        assert np.abs(np.median(vel, axis=0) * 0.05 * cam["fx"] - flow).max() < 0.2       # the flow again, in px per image; the median bears the few moved points
    t.close(); e.close()
