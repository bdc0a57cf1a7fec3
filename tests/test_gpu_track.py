"""include/viltrack.h on the GPU against tests/track_ref.py, on raw bytes: pyramid levels, LK results with their per-level termination
codes and iteration counts, setMask, the corner response, the candidates and the picks with their order.  No tolerance anywhere: every sum
of the contract is an integer sum and the few float32 operations are unfused IEEE in a fixed order."""
import functools
import hashlib
import os
import subprocess
import sys

import numpy as np
import pytest

import track_fixtures as tf
import track_ref as tr
from mvil_fusion_amd import lib, track

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
F32 = np.float32
NONE = np.zeros((0, 2), F32)


@pytest.fixture(scope="module")
def so():
    return lib.load_vilsolve()


def same(a, b, what):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.dtype == b.dtype and a.shape == b.shape, (what, a.dtype, b.dtype, a.shape, b.shape)
    if a.tobytes() != b.tobytes():
        bad = np.flatnonzero((a.view(np.uint8).reshape(len(a), -1) != b.view(np.uint8).reshape(len(b), -1)).any(axis=1)) if a.ndim and len(a) else []
        raise AssertionError("%s differs in %d rows, first %s: device %s, restatement %s" % (what, len(bad), bad[:5], a[bad[:3]] if len(bad) else a, b[bad[:3]] if len(bad) else b))


@functools.lru_cache(maxsize=None)
def lk_reference(height, width, max_level):
    """the restatement on the branch-covering set, computed once"""
    cur, forw = tf.parity_pair(height, width)
    return tr.track(tr.pyramid(cur, max_level), tr.pyramid(forw, max_level), tf.parity_points(height, width), max_level)[:4]


def test_pyramid_levels_equal_the_restatement(so):
    img = track.Texture(97, 131, seed=4).render(noise=6.0)
    t = track.Tracker(so, 131, 97, max_level=3, max_points=8, max_candidates=1024)
    padded = np.zeros((97, 160), np.uint8); padded[:, :131] = img; padded[:, 131:] = 200          # a row stride wider than the image
    t.push_image(padded, row_stride=160)
    ref = tr.pyramid(img, 3)
    assert [r.shape for r in ref] == [(97, 131), (49, 66), (25, 33), (13, 17)]
    for l in range(4):
        same(t.debug_level("forw", l), ref[l], "forw level %d" % l)
        same(t.debug_level("cur", l), ref[l], "cur level %d (first image: cur = forw)" % l)
    img2 = track.Texture(97, 131, seed=5).render()
    t.push_image(img2)
    ref2 = tr.pyramid(img2, 3)
    for l in range(4):
        same(t.debug_level("forw", l), ref2[l], "second forw level %d" % l)
        same(t.debug_level("cur", l), ref[l], "second cur level %d" % l)
    t.close()


@pytest.mark.parametrize("height,width,max_level", tf.SETUPS)
def test_lk_equals_the_restatement_on_the_branch_covering_set(so, height, width, max_level):
    cur, forw = tf.parity_pair(height, width)
    pts = tf.parity_points(height, width)
    r_out, r_st, r_codes, r_iters = lk_reference(height, width, max_level)
    t = track.Tracker(so, width, height, max_level=max_level, max_points=len(pts), max_candidates=1024)
    t.push_image(cur); t.push_image(forw)
    out, st, s = t.track(pts)                               # n = max_points
    codes, iters = t.debug_lk()
    same(codes, r_codes, "termination codes"); same(iters, r_iters, "iteration counts")
    same(st, r_st, "status"); same(out, r_out, "forw_xy")
    assert (s.n_points, s.n_tracked) == (len(pts), int(r_st.sum()))
    for i in (0, 60, len(pts) - 1):                         # n = 1: the same point alone gives the same bytes
        o1, s1, _ = t.track(pts[i:i + 1])
        c1, i1 = t.debug_lk()
        same(o1, r_out[i:i + 1], "forw_xy of point %d alone" % i); same(s1, r_st[i:i + 1], "status alone"); same(c1, r_codes[i:i + 1], "codes alone"); same(i1, r_iters[i:i + 1], "iters alone")
    o0, s0, sm = t.track(NONE)
    assert len(o0) == 0 and len(s0) == 0 and sm.n_points == 0
    t.close()


def both_detect(t, img, tracks, min_dist, max_cnt, quality=0.01):
    kept, new, s = t.detect(tracks, min_dist, max_cnt, quality)
    eig, mask, n_cand = t.debug_detect()
    r_kept, r_new, r_eig, r_mask, r_ncand = tr.detect(img, tracks, min_dist, max_cnt, quality)
    same(eig, r_eig, "eig map"); same(mask, r_mask, "mask")
    assert n_cand == r_ncand == s.n_candidates
    same(kept, r_kept, "kept"); same(new, r_new, "new_xy")
    assert (s.n_tracks, s.n_kept, s.n_new) == (len(tracks), int(r_kept.sum()), len(r_new))
    return kept, new, s


@pytest.mark.parametrize("height,width,min_dist,max_cnt", ((96, 128, 10, 30), (192, 256, 30, 150)))
def test_detector_equals_the_restatement(so, height, width, min_dist, max_cnt):
    t = track.Tracker(so, width, height, max_level=1, max_points=256, max_candidates=height * width)
    rng = np.random.default_rng(3)
    noisy, tiled, clean = tf.noisy_image(height, width), tf.tiled_image(height, width), tf.clean_image(height, width)
    t.push_image(noisy)
    kept, new, s = both_detect(t, noisy, NONE, min_dist, max_cnt)                                    # n_tracks = 0
    assert s.n_picked >= s.n_new > 0
    # tracks that suppress each other, one outside, one non-finite; the picks of the empty call as tracks
    tracks = np.concatenate([new[:5], new[:5] + F32(0.4), [[-3.0, 5.0], [np.nan, 4.0], [width - 0.6, 10.0], [width - 0.4, 10.0]], new[5:9] + [[min_dist, 0.0]]]).astype(F32)
    kept, new2, s = both_detect(t, noisy, tracks, min_dist, max_cnt)
    assert kept[0] == 1 and not kept[5:10].any() and kept[10:12].tolist() == [0, 0] and kept[13] == 0       # same pixel as an earlier track; outside; NaN; rounds to x = width
    many = np.stack([rng.uniform(0, width - 1, 256), rng.uniform(0, height - 1, 256)], axis=1).astype(F32)
    _, none, s = both_detect(t, noisy, many, 2, 20)                                                  # n_kept >= max_cnt: no new points
    assert s.n_kept >= 20 and len(none) == 0 and s.n_candidates > 0
    _, cut, s = both_detect(t, noisy, NONE, min_dist, 7)                                             # the max_cnt cut ends the picks early
    assert len(cut) == 7 and s.n_picked > 7
    same(cut, new[:7], "the cut is a prefix of the uncut picks")
    both_detect(t, noisy, many[:40], 0, 50)                                                          # min_dist 0: only equal pixels collide
    t.push_image(tiled)
    _, tn, s = both_detect(t, tiled, NONE, min_dist, 10 * max_cnt)                                   # equal responses: ties by pixel index
    e = tr.corner_response(tiled)[tn[:, 1].astype(int), tn[:, 0].astype(int)]
    assert (np.diff(e) == 0).any()
    t.push_image(clean)
    both_detect(t, clean, many[:100], min_dist, max_cnt, quality=0.05)
    t.close()


def run_chain(so, on_image=None):
    """six 96 x 128 images with a drifting shift: push, track, compact on status, detect, append.  Returns the digest of every output."""
    images, _ = track.sequence(96, 128, 6, seed=2)
    t = track.Tracker(so, 128, 96, max_level=2, max_points=256, max_candidates=96 * 128)
    h = hashlib.sha256()
    pts = NONE
    for k, img in enumerate(images):
        t.push_image(img)
        out, st, _ = t.track(pts)
        pts = out[st == 1]
        kept, new, _ = t.detect(pts, 10, 60, 0.01)
        if on_image:
            on_image(k, out, st, kept, new)
        pts = np.concatenate([pts[kept == 1], new])
        # the first image, tracked against itself once it has points, must not move them
        if k == 0:
            o0, s0, _ = t.track(pts)
            assert o0.tobytes() == pts.tobytes() and s0.all(), "the first image is cur and forw: zero flow"
        for a in (out, st, kept, new):
            h.update(np.ascontiguousarray(a).tobytes())
    t.close()
    return h.hexdigest()


def test_resident_chain_equals_the_restatement_at_every_image(so):
    images, shifts = track.sequence(96, 128, 6, seed=2)
    ref = tr.RefTracker(2)
    state = {"pts": NONE, "seen": 0, "tracked": 0}

    def check(k, out, st, kept, new):
        ref.push(images[k])
        r_out, r_st = ref.track(state["pts"])[:2]
        same(st, r_st, "status at image %d" % k); same(out, r_out, "points at image %d" % k)
        p = r_out[r_st == 1]
        r_kept, r_new = ref.detect(p, 10, 60)[:2]
        same(kept, r_kept, "kept at image %d" % k); same(new, r_new, "new points at image %d" % k)
        if k:                                               # and the chain follows the texture: a stale pyramid or a wrong swap would not
            flow = (r_out - state["pts"])[r_st == 1]
            true = np.array(shifts[k]) - np.array(shifts[k - 1])
            assert len(flow) > 20 and np.abs(np.median(flow, axis=0) - true).max() < 0.1, (k, np.median(flow, axis=0), true)
        state["pts"] = np.concatenate([p[r_kept == 1], r_new]); state["seen"] += 1; state["tracked"] += int(r_st.sum())
    run_chain(so, check)
    assert state["seen"] == 6 and state["tracked"] > 150


def test_bit_reproducible_across_runs_and_processes(so):
    a = run_chain(so)
    assert run_chain(so) == a
    out = subprocess.run([sys.executable, os.path.join(HERE, "track_child.py")], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr[-2000:]
    child = [l for l in out.stdout.splitlines() if l.startswith("digest ")]
    assert child == ["digest " + a], (child, a)


def test_errors_write_nothing_and_leave_the_images_resident(so):
    height, width, max_level = tf.SETUPS[0]
    cur, forw = tf.parity_pair(height, width)
    pts = tf.parity_points(height, width)
    r_out, r_st, r_codes, r_iters = lk_reference(height, width, max_level)
    n_cand = tr.detect(forw, pts[:8], 10, 30, 0.01)[4]
    assert n_cand > 8
    t = track.Tracker(so, width, height, max_level=max_level, max_points=len(pts), max_candidates=n_cand - 1)
    with pytest.raises(track.TrackError) as e:              # no image yet
        t.track(pts[:4])
    assert e.value.status == -1
    t.push_image(cur); t.push_image(forw)
    with pytest.raises(track.TrackError) as e:              # a stride narrower than the image: forw and cur stay
        t.push_image(np.zeros((height, width), np.uint8), row_stride=width - 1)
    assert e.value.status == -1
    fo = np.full((len(pts) + 1, 2), 7.0, F32); so_ = np.full(len(pts) + 1, 9, np.uint8)
    with pytest.raises(track.TrackError) as e:              # n > max_points
        t.track(np.concatenate([pts, pts[:1]]), forw_out=fo, status_out=so_)
    assert e.value.status == -1 and (fo == 7.0).all() and (so_ == 9).all()
    ko = np.full(8, 9, np.uint8); no = np.full((30, 2), 7.0, F32)
    with pytest.raises(track.TrackError) as e:              # one candidate more than there is room for
        t.detect(pts[:8], 10, 30, kept_out=ko, new_out=no)
    assert e.value.status == -6 and (ko == 9).all() and (no == 7.0).all()
    with pytest.raises(track.TrackError) as e:
        t.detect(np.concatenate([pts, pts[:1]]), 10, 30, kept_out=ko, new_out=no)
    assert e.value.status == -1 and (ko == 9).all() and (no == 7.0).all()
    for bad in (dict(min_dist=-1), dict(max_cnt=-1), dict(quality=0.0), dict(quality=float("nan")), dict(min_dist=1025)):
        with pytest.raises(track.TrackError) as e:
            t.detect(pts[:8], **dict(dict(min_dist=10, max_cnt=30, quality=0.01), **bad))
        assert e.value.status == -1, bad
    out, st, _ = t.track(pts)                               # the next valid call still matches
    same(out, r_out, "forw_xy after the errors"); same(st, r_st, "status after the errors")
    same(t.debug_level("cur", 1), tr.pyramid(cur, 1)[1], "cur after the errors"); same(t.debug_level("forw", 0), forw, "forw after the errors")
    t.close()
