"""NumPy restatement of include/vilclahe.h's arithmetic contract (CLAHE on 8-bit images), step by step as the header numbers them.
Integers are int64, f32 is numpy.float32 one operation at a time.  Shares no code with mvil-fusion_amd/clahe.py; the device is compared
with it on raw bytes.  OpenCV is not on these machines: nothing here is checked against OpenCV's bits."""
import numpy as np

F = np.float32


def r101(i, n):
    """reflect-101 index of any integer (array) i into [0, n)"""
    i = np.asarray(i, np.int64)
    if n == 1:
        return np.zeros_like(i)
    p = 2 * (n - 1)
    i = np.mod(i, p)
    return np.where(i >= n, p - i, i)


# ---- steps 1 and 2 --------------------------------------------------------------------------------------------------------------
def geometry(height, width, tiles_x, tiles_y, clip_limit):
    """dict: he, we (the extended size), th, tw, area, clip, lut_scale, inv_tw, inv_th"""
    we, he = width, height
    if width % tiles_x or height % tiles_y:                 # both sides are padded whenever either is not divisible
        we, he = width + tiles_x - width % tiles_x, height + tiles_y - height % tiles_y
    tw, th = we // tiles_x, he // tiles_y
    area = tw * th
    clip = 0 if clip_limit == 0 else max(int(float(clip_limit) * area / 256), 1)
    return dict(he=he, we=we, th=th, tw=tw, area=area, clip=clip, lut_scale=F(F(255.0) / F(area)), inv_tw=F(F(1.0) / F(tw)), inv_th=F(F(1.0) / F(th)))


def extended(img, g):
    h, w = img.shape
    return img[np.ix_(r101(np.arange(g["he"]), h), r101(np.arange(g["we"]), w))]


# ---- step 3 ---------------------------------------------------------------------------------------------------------------------
def tile_lut(tile, g):
    """(hist after clipping and redistribution int64[256], lut uint8[256], stats) of one tile of the extended image"""
    hist = np.bincount(tile.ravel(), minlength=256).astype(np.int64)
    clip = g["clip"]
    stats = dict(clipped=0, batch=0, residual=0, step=0)
    if clip > 0:
        clipped = int(np.maximum(hist - clip, 0).sum())
        hist = np.minimum(hist, clip)
        batch = clipped // 256
        residual = clipped - 256 * batch
        hist = hist + batch
        step = 0
        if residual > 0:
            step = max(256 // residual, 1)
            i = np.arange(256)
            hist = hist + ((i % step == 0) & (i // step < residual)).astype(np.int64)
        stats = dict(clipped=clipped, batch=batch, residual=residual, step=step)
    lut = np.clip(np.rint(np.cumsum(hist).astype(F) * g["lut_scale"]), 0, 255).astype(np.uint8)
    return hist, lut, stats


def luts(img, tiles_x=8, tiles_y=8, clip_limit=3.0):
    """(hists [tiles_y][tiles_x][256] int32, luts the same uint8, stats [tiles_y][tiles_x] dicts, geometry)"""
    img = np.asarray(img, np.uint8)
    g = geometry(img.shape[0], img.shape[1], tiles_x, tiles_y, clip_limit)
    ext = extended(img, g)
    hists = np.zeros((tiles_y, tiles_x, 256), np.int32); L = np.zeros((tiles_y, tiles_x, 256), np.uint8)
    stats = [[None] * tiles_x for _ in range(tiles_y)]
    for ty in range(tiles_y):
        for tx in range(tiles_x):
            h, l, s = tile_lut(ext[ty * g["th"]:(ty + 1) * g["th"], tx * g["tw"]:(tx + 1) * g["tw"]], g)
            hists[ty, tx] = h; L[ty, tx] = l; stats[ty][tx] = s
    return hists, L, stats, g


# ---- step 4 ---------------------------------------------------------------------------------------------------------------------
def _axis(n, inv, tiles, fused):
    x = np.arange(n).astype(F)
    if fused:
        tf = (x.astype(np.float64) * np.float64(inv) - 0.5).astype(F)                               # fma(x, inv, -0.5): one rounding
    else:
        tf = (x * inv) - F(0.5)
    fl = np.floor(tf)
    a = tf - fl
    a1 = F(1.0) - a
    t1 = fl.astype(np.int64)
    return np.maximum(t1, 0), np.minimum(t1 + 1, tiles - 1), a, a1


def _fma(p, q, r):
    """p * q + r rounded once (the product of two float32 is exact in float64)"""
    return (p.astype(np.float64) * q.astype(np.float64) + r.astype(np.float64)).astype(F)


def blend(img, L, g, fused=False):
    img = np.asarray(img, np.uint8)
    h, w = img.shape
    tiles_y, tiles_x = L.shape[:2]
    tx1, tx2, xa, xa1 = _axis(w, g["inv_tw"], tiles_x, fused)
    ty1, ty2, ya, ya1 = _axis(h, g["inv_th"], tiles_y, fused)
    v = img.astype(np.int64)
    Y1, Y2, X1, X2 = ty1[:, None], ty2[:, None], tx1[None, :], tx2[None, :]
    l11, l12, l21, l22 = (L[Y1, X1, v].astype(F), L[Y1, X2, v].astype(F), L[Y2, X1, v].astype(F), L[Y2, X2, v].astype(F))
    XA, XA1, YA, YA1 = (np.broadcast_to(xa[None, :], (h, w)), np.broadcast_to(xa1[None, :], (h, w)), np.broadcast_to(ya[:, None], (h, w)),
                        np.broadcast_to(ya1[:, None], (h, w)))
    if fused:                                               # a * b + c * d contracts to fma(a, b, c * d)
        top = _fma(l11, XA1, l12 * XA); bot = _fma(l21, XA1, l22 * XA)
        res = _fma(top, YA1, bot * YA)
    else:
        top = (l11 * XA1) + (l12 * XA); bot = (l21 * XA1) + (l22 * XA)
        res = (top * YA1) + (bot * YA)
    assert res.dtype == F
    return np.clip(np.rint(res), 0, 255).astype(np.uint8)


def apply(img, tiles_x=8, tiles_y=8, clip_limit=3.0, fused=False, full=False):
    """the equalised image; full=True: (image, hists, luts, stats, geometry)"""
    hists, L, stats, g = luts(img, tiles_x, tiles_y, clip_limit)
    out = blend(img, L, g, fused)
    return (out, hists, L, stats, g) if full else out
