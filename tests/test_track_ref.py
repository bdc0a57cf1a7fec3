"""tests/track_ref.py (the NumPy restatement of include/viltrack.h) on its own, no GPU: LK against an analytically shifted texture, the
branch coverage of the point set the GPU parity test uses, and the detector's defining properties."""
import numpy as np
import pytest

import track_fixtures as tf
import track_ref as tr
from mvil_fusion_amd import track

F32 = np.float32
GROUND_TRUTH = ((96, 128, 1, (1.3, -0.7)), (96, 128, 1, (3.6, 2.2)), (192, 256, 3, (1.3, -0.7)), (192, 256, 3, (5.4, -3.2)))


@pytest.mark.parametrize("height,width,max_level,shift", GROUND_TRUTH)
def test_lk_restatement_recovers_a_known_subpixel_shift(height, width, max_level, shift):
    tex = track.Texture(height, width, seed=0)
    margin = 14 + int(np.ceil(np.hypot(*shift)))
    pts = track.interior_points(height, width, 60, margin, seed=1)
    out, status, codes, iters, _ = tr.track(tr.pyramid(tex.render(), max_level), tr.pyramid(tex.render(shift), max_level), pts, max_level)
    err = np.abs(out.astype(np.float64) - (pts.astype(np.float64) + np.array(shift))).max(axis=1)
    print("worst %.4f px, median %.4f px" % (err.max(), np.median(err)))
    assert status.tolist() == [1] * 60
    assert err.max() < 0.1                                  # this restatement reaches 0.015 / 0.024 / 0.029 / 0.028 px worst on the four setups (median 0.005 - 0.008)


@pytest.mark.parametrize("height,width,max_level", tf.SETUPS)
def test_parity_point_set_leaves_the_main_branch(height, width, max_level):
    """The set test_gpu_track.py compares on takes every exit of steps 3-6.  D < FLT_EPSILON without minEig < 1e-4 cannot happen (minEig
    >= 1e-4 puts both eigenvalues above 0.088, so D above 0.0077): the flat patch meets both conditions of step 4 at once."""
    cur, forw = tf.parity_pair(height, width)
    pts = tf.parity_points(height, width)
    assert 90 <= len(pts) <= 110
    out, status, codes, iters, causes = tr.track(tr.pyramid(cur, max_level), tr.pyramid(forw, max_level), pts, max_level)
    for name, code in (("EPS", tr.EPS), ("OSC", tr.OSC), ("CAP", tr.CAP), ("OOB", tr.OOB), ("SKIP", tr.SKIP), ("LOWEIG", tr.LOWEIG)):
        assert (codes == code).any(), name
    assert {"EPS", "OSC", "CAP", "OOB", "mineig0", "det0", "skip0", "skip_upper", "border"} <= causes, sorted(causes)
    assert (iters[codes == tr.CAP] == 30).all() and (iters[codes == tr.OSC] >= 2).all() and (iters[(codes == tr.SKIP) | (codes == tr.LOWEIG)] == 0).all()
    assert 0 < status.sum() < len(pts)
    frac = pts - np.floor(pts)
    assert (frac == 0).all(axis=1).sum() >= 5               # a = b = 0
    assert ((pts < -20).any(axis=1) | (pts[:, 0] > width + 20) | (pts[:, 1] > height + 20)).sum() >= 4
    assert np.isfinite(out).all()


def test_pyramid_sizes_and_constant_image():
    img = np.full((97, 131), 77, np.uint8)
    levels = tr.pyramid(img, 3)
    assert [l.shape for l in levels] == [(97, 131), (49, 66), (25, 33), (13, 17)]
    assert all((l == 77).all() for l in levels)
    assert tr.r101(np.array([-3, -1, 0, 4, 5, 6, 9, -9]), 5).tolist() == [3, 1, 0, 4, 3, 2, 1, 1]


@pytest.mark.parametrize("image,min_dist,max_cnt", (("noisy", 10, 30), ("clean", 10, 500), ("tiled", 10, 500)))
def test_detector_picks_are_apart_unmasked_and_ordered(image, min_dist, max_cnt):
    img = getattr(tf, image + "_image")(96, 128)
    tracks = np.array([[30.2, 40.7], [33.0, 44.0], [100.0, 20.0], [-5.0, 3.0], [99.6, 20.4], [64.0, 90.0]], F32)
    kept, new, eig, mask, n_cand = tr.detect(img, tracks, min_dist, max_cnt, 0.01)
    assert kept.tolist() == [1, 0, 1, 0, 0, 1]
    assert len(new) == min(max_cnt - 3, len(new)) and len(new) > 10 and n_cand >= len(new)
    d2 = ((new[:, None, :] - new[None, :, :]) ** 2).sum(axis=2) + 1e9 * np.eye(len(new))
    assert d2.min() >= min_dist * min_dist
    xi, yi = new[:, 0].astype(int), new[:, 1].astype(int)
    assert (mask[yi, xi] == 255).all()
    assert (mask[41, 30] == 0) and (mask[41, 40] == 0) and (mask[41, 41] == 255)          # the exact disc: (30, 41) +- 10
    e = eig[yi, xi]
    assert (np.diff(e) <= 0).all()                          # pick order follows the rank
    if max_cnt == 30:
        assert len(new) == 27                               # the max_cnt cut ends the picks


def test_detector_ties_go_to_the_lower_pixel_index():
    img = tf.tiled_image(96, 128)
    kept, new, eig, mask, n_cand = tr.detect(img, np.zeros((0, 2), F32), 10, 500, 0.01)
    ranked, _ = tr.candidates(eig, mask, 0.01)
    e = eig.ravel()[ranked]
    ties = np.flatnonzero(np.diff(e) == 0)
    assert len(ties) > 20, "the tiled image must force equal responses"
    assert (np.diff(ranked)[ties] > 0).all()
    p = (new[:, 1] * 128 + new[:, 0]).astype(np.int64); pe = eig.ravel()[p]
    same = np.flatnonzero(np.diff(pe) == 0)
    assert len(same) > 0 and (np.diff(p)[same] > 0).all()
