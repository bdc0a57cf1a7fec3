"""Inputs the CLAHE tests share: the images and the (shape, tiles, clip limit) cases that tests/test_clahe_ref.py proves to cover the
branches of include/vilclahe.h's contract on the CPU and tests/test_gpu_clahe.py compares the device on; the restatement's answers are
computed once per case."""
import functools

import numpy as np

import clahe_ref as cr
from mvil_fusion_amd import track

# height, width, tiles_x, tiles_y, clip_limit
CASES = (
    (16, 16, 8, 8, 3.0),        # the smallest legal image: 2 x 2-pixel tiles, clip 1
    (48, 64, 8, 8, 3.0),
    (50, 64, 8, 8, 3.0),        # rows padded; columns padded by a full 8
    (48, 67, 8, 8, 3.0),        # columns padded; rows by a full 8; width no multiple of 4
    (61, 75, 8, 8, 3.0),        # both
    (192, 256, 8, 8, 3.0),      # 32 x 24 tiles, one of them flat: batch 2
    (48, 64, 2, 2, 3.0),
    (48, 64, 1, 1, 3.0),        # one tile of 3072 pixels: three workgroups' shares
    (48, 64, 3, 5, 3.0),
    (48, 64, 8, 8, 0.0),        # no clipping
    (48, 64, 8, 8, 40.0),       # OpenCV's default, the stereo branch
    (480, 640, 8, 8, 3.0),      # the camera's: 80 x 60 tiles, five shares each
)


@functools.lru_cache(maxsize=None)
def image(height, width, seed=21):
    """a noisy sum of sinusoids with a flat patch of up to 40 x 40 from (width // 8, height // 8)"""
    img = track.Texture(height, width, seed=seed).render(noise=8.0, seed=seed + 1)
    fy, fx, ph, pw = height // 8, width // 8, min(40, height // 4), min(40, width // 4)
    img[fy:fy + ph, fx:fx + pw] = 128
    img.setflags(write=False)
    return img


@functools.lru_cache(maxsize=None)
def reference(height, width, tiles_x, tiles_y, clip_limit, seed=21):
    """(equalised image, hists, luts, stats, geometry) of the restatement on image(height, width, seed); read-only"""
    out = cr.apply(image(height, width, seed), tiles_x, tiles_y, clip_limit, full=True)
    for a in out[:3]:
        a.setflags(write=False)
    return out
