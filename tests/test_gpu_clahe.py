"""include/vilclahe.h on the GPU against tests/clahe_ref.py, on raw bytes: the equalised image, the LUTs and the histograms after clipping
and redistribution of vclahe_apply, and the tracker that vclahe_push leaves behind against host CLAHE followed by vtrack_push_image.  No
tolerance anywhere: the histogram work is integer and the blend is four unfused float32 terms in a fixed order.

k_clahe_hist gives a workgroup a share of at least 1024 pixels of a tile.  Of the cases of tests/clahe_fixtures.py, (48, 64) at tiles 1 x 1
(one tile of 3072 pixels, three shares) and (480, 640) at 8 x 8 (4800 pixels a tile, five shares of 960) make a tile span more than one
workgroup's share; every other case has one workgroup per tile."""
import ctypes as C
import hashlib
import os
import subprocess
import sys

import numpy as np
import pytest

import clahe_fixtures as cf
import clahe_ref as cr
import track_fixtures as tf
import track_ref as tr
from mvil_fusion_amd import clahe, lib, track

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
F32 = np.float32


@pytest.fixture(scope="module")
def so():
    return lib.load_vilsolve()


def same(a, b, what):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.dtype == b.dtype and a.shape == b.shape, (what, a.dtype, b.dtype, a.shape, b.shape)
    if a.tobytes() != b.tobytes():
        bad = np.argwhere(a != b)
        raise AssertionError("%s differs at %d places, first %s: device %s, expected %s" % (what, len(bad), bad[:5].tolist(), a[tuple(bad[:5].T)], b[tuple(bad[:5].T)]))


def same_levels(a, b, max_level, what):
    for which in ("cur", "forw"):
        for l in range(max_level + 1):
            same(a.debug_level(which, l), b.debug_level(which, l), "%s: %s level %d" % (what, which, l))


@pytest.mark.parametrize("case", cf.CASES, ids=lambda c: "%dx%d-tiles%dx%d-clip%g" % c)
def test_apply_equals_the_restatement(so, case):
    height, width, tiles_x, tiles_y, clip = case
    r_out, r_hist, r_lut, _, _ = cf.reference(*case)
    c = clahe.Clahe(so, width, height, tiles_x, tiles_y, clip)
    out = c.apply(cf.image(height, width))
    same(c.debug_hist(), r_hist, "histograms after redistribution")
    same(c.debug_lut(), r_lut, "LUTs")
    same(out, r_out, "equalised image")
    c.close()


def test_a_flat_and_a_saturated_image(so):
    """every wave of k_clahe_hist meets 64 equal pixels: one bin holds the whole tile, the clip hands it out again"""
    c = clahe.Clahe(so, 64, 48)
    for v in (0, 128, 255):
        img = np.full((48, 64), v, np.uint8)
        r_out, r_hist, r_lut, _, _ = cr.apply(img, full=True)
        same(c.apply(img), r_out, "flat %d" % v); same(c.debug_hist(), r_hist, "histograms of flat %d" % v); same(c.debug_lut(), r_lut, "LUTs of flat %d" % v)
    c.close()


@pytest.mark.parametrize("height,width,max_level", tf.SETUPS)
def test_push_equals_host_clahe_then_push_image(so, height, width, max_level):
    pts = tf.parity_points(height, width)
    a = track.Tracker(so, width, height, max_level=max_level, max_points=len(pts), max_candidates=height * width)
    b = track.Tracker(so, width, height, max_level=max_level, max_points=len(pts), max_candidates=height * width)
    c = clahe.Clahe(so, width, height)
    eq = []
    for k, raw in enumerate(tf.parity_pair(height, width)):
        E = cr.apply(raw)
        eq.append(E)
        out = c.push(a, raw, want_equalised=True)
        b.push_image(E)
        same(out, E, "out of push %d" % k); same(c.apply(raw), out, "apply against push %d" % k)
        same_levels(a, b, max_level, "after image %d" % k)
        ref = tr.pyramid(E, max_level)
        for l in range(max_level + 1):
            same(a.debug_level("forw", l), ref[l], "forw level %d of image %d against the restatement" % (l, k))
            same(a.debug_level("cur", l), tr.pyramid(eq[0], max_level)[l], "cur level %d after image %d" % (l, k))
    oa, sa, _ = a.track(pts); ca, ia = a.debug_lk()
    ob, sb, _ = b.track(pts); cb, ib = b.debug_lk()
    same(oa, ob, "forw_xy"); same(sa, sb, "status"); same(ca, cb, "termination codes"); same(ia, ib, "iteration counts")
    assert sa.sum() > 20
    ka, na, ma = a.detect(oa[sa == 1], 10, 60)
    kb, nb, mb = b.detect(ob[sb == 1], 10, 60)
    same(ka, kb, "kept"); same(na, nb, "picks")
    assert len(na) > 0 and (ma.n_kept, ma.n_candidates, ma.n_picked) == (mb.n_kept, mb.n_candidates, mb.n_picked)
    assert c.push(a, tf.parity_pair(height, width)[0]) is None                                       # without the read-back
    b.push_image(eq[0])
    same_levels(a, b, max_level, "after a push without out")
    for h in (a, b, c):
        h.close()


def test_a_row_stride_wider_than_the_image(so):
    height, width = 50, 67
    img = cf.image(height, width)
    r_out = cr.apply(img)
    wide = np.full((height, 96), 200, np.uint8); wide[:, :width] = img
    c = clahe.Clahe(so, width, height)
    same(c.apply(wide, row_stride=96), r_out, "apply from a wide image")
    out = np.full((height, 80), 9, np.uint8)
    c.apply(wide, row_stride=96, out=out[:, :width])                                                # and into one
    same(out[:, :width], r_out, "apply into a wide image"); assert (out[:, width:] == 9).all()
    a = track.Tracker(so, width, height, max_level=2, max_points=8, max_candidates=1024)
    same(c.push(a, wide, want_equalised=True, row_stride=96), r_out, "push from a wide image")
    for l, lv in enumerate(tr.pyramid(r_out, 2)):
        same(a.debug_level("forw", l), lv, "level %d" % l)
    a.close(); c.close()


def test_errors_leave_the_tracker_and_the_outputs_alone(so):
    height, width, max_level = tf.SETUPS[0]
    cur, forw = tf.parity_pair(height, width)
    pts = tf.parity_points(height, width)
    a = track.Tracker(so, width, height, max_level=max_level, max_points=len(pts), max_candidates=1024)
    c = clahe.Clahe(so, width, height)
    wider, taller = clahe.Clahe(so, width + 16, height), clahe.Clahe(so, width, height + 16)
    push = so.vclahe_push; push.restype = C.c_int

    def failures():
        with pytest.raises(clahe.ClaheError) as e:          # a tracker of another size
            wider.push(a, np.zeros((height, width + 16), np.uint8))
        assert e.value.status == -1
        with pytest.raises(clahe.ClaheError) as e:
            taller.push(a, np.zeros((height + 16, width), np.uint8))
        assert e.value.status == -1
        with pytest.raises(clahe.ClaheError) as e:          # a stride narrower than the image
            c.push(a, np.zeros((height, width), np.uint8), row_stride=width - 1)
        assert e.value.status == -1
        assert push(c.ctx, a.ctx, None, C.c_int32(width), None, C.c_int32(0)) == -1                  # no image
        assert push(c.ctx, None, C.c_void_p(cur.ctypes.data), C.c_int32(width), None, C.c_int32(0)) == -1          # no tracker
        out = np.full((height, width), 9, np.uint8)
        assert push(c.ctx, a.ctx, C.c_void_p(cur.ctypes.data), C.c_int32(width), C.c_void_p(out.ctypes.data), C.c_int32(width - 1)) == -1
        assert (out == 9).all()
        with pytest.raises(clahe.ClaheError) as e:
            c.apply(cur, row_stride=width - 1, out=out)
        assert e.value.status == -1 and (out == 9).all()

    failures()                                              # before the first image: the tracker still has none
    with pytest.raises(track.TrackError) as e:
        a.track(pts[:4])
    assert e.value.status == -1
    with pytest.raises(clahe.ClaheError) as e:              # nothing to read yet
        c.debug_lut()
    assert e.value.status == -1
    c.push(a, cur); c.push(a, forw)
    levels = [(w, l, a.debug_level(w, l)) for w in ("cur", "forw") for l in range(max_level + 1)]
    o0, s0, _ = a.track(pts)
    same(levels[0][2], cr.apply(cur), "cur"); same(levels[max_level + 1][2], cr.apply(forw), "forw")
    failures()
    for w, l, lv in levels:
        same(a.debug_level(w, l), lv, "%s level %d after the errors" % (w, l))
    o1, s1, _ = a.track(pts)
    same(o1, o0, "forw_xy after the errors"); same(s1, s0, "status after the errors")
    for h in (a, c, wider, taller):
        h.close()


def test_push_image_and_clahe_push_alternate_on_one_tracker(so):
    height, width, max_level = 96, 128, 2
    images, _ = track.sequence(height, width, 4, seed=5, noise=4.0)
    a = track.Tracker(so, width, height, max_level=max_level, max_points=8, max_candidates=1024)
    b = track.Tracker(so, width, height, max_level=max_level, max_points=8, max_candidates=1024)
    c = clahe.Clahe(so, width, height)
    for k, raw in enumerate(images):
        E = cr.apply(raw)
        if k % 2:
            c.push(a, raw)
        else:
            a.push_image(E)
        b.push_image(E)
        same_levels(a, b, max_level, "image %d" % k)
        same(a.debug_level("forw", 0), E, "forw of image %d" % k)
    for h in (a, b, c):
        h.close()


def test_the_profile_counts_one_launch_per_kernel(so):
    height, width = 96, 128
    a = track.Tracker(so, width, height, max_level=3, max_points=8, max_candidates=1024)
    c = clahe.Clahe(so, width, height)
    c.profile_enable(True); a.profile_enable(True)
    c.apply(cf.image(height, width))
    p = c.profile_read()
    assert [p[k][0] for k in clahe.KERNELS] == [1, 1, 1] and all(p[k][1] > 0.0 for k in clahe.KERNELS), p
    c.push(a, cf.image(height, width))
    p, q = c.profile_read(), a.profile_read()
    assert [p[k][0] for k in clahe.KERNELS] == [1, 1, 1] and q["k_track_pyr"][0] == 3, (p, q)
    c.profile_enable(False)
    c.apply(cf.image(height, width))
    assert [v[0] for v in c.profile_read().values()] == [0, 0, 0]
    a.close(); c.close()


def run_chain(so):
    """four 96 x 128 raw images: equalised into the tracker, tracked, detected.  Returns the digest of every output."""
    images, _ = track.sequence(96, 128, 4, seed=3, noise=3.0)
    t = track.Tracker(so, 128, 96, max_level=2, max_points=256, max_candidates=96 * 128)
    c = clahe.Clahe(so, 128, 96)
    h = hashlib.sha256()
    pts = np.zeros((0, 2), F32)
    for img in images:
        E = c.push(t, img, want_equalised=True)
        out, st, _ = t.track(pts)
        pts = out[st == 1]
        kept, new, _ = t.detect(pts, 10, 60, 0.01)
        pts = np.concatenate([pts[kept == 1], new])
        for a in (E, c.debug_hist(), c.debug_lut(), c.apply(img), out, st, kept, new):
            h.update(np.ascontiguousarray(a).tobytes())
    t.close(); c.close()
    return h.hexdigest()


def test_bit_reproducible_across_calls_and_processes(so):
    a = run_chain(so)
    assert run_chain(so) == a
    out = subprocess.run([sys.executable, os.path.join(HERE, "clahe_child.py")], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr[-2000:]
    child = [l for l in out.stdout.splitlines() if l.startswith("digest ")]
    assert child == ["digest " + a], (child, a)
