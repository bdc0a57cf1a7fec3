"""NumPy restatement of include/viltrack.h's arithmetic contract (pyramidal LK tracking, setMask, min-eigenvalue corners), step by step
as the header numbers them.  Integers are int64, f32 is numpy.float32 one operation at a time.  Shares no code with
mvil-fusion_amd/track.py; the device is compared with it on raw bytes."""
import numpy as np

F = np.float32
WIN, HALF, MAX_ITERS = 21, F(10.0), 30
SKIP, LOWEIG, EPS, OSC, CAP, OOB = 0, 1, 2, 3, 4, 5
CODE_NAMES = {SKIP: "SKIP", LOWEIG: "LOWEIG", EPS: "EPS", OSC: "OSC", CAP: "CAP", OOB: "OOB"}
FLT_EPSILON = F(np.finfo(np.float32).eps)
S20 = F(2.0 ** -20)


def r101(i, n):
    """reflect-101 index of any integer (array) i into [0, n)"""
    i = np.asarray(i, np.int64)
    if n == 1:
        return np.zeros_like(i)
    p = 2 * (n - 1)
    i = np.mod(i, p)
    return np.where(i >= n, p - i, i)


# ---- step 1 ---------------------------------------------------------------------------------------------------------------------
def pyr_down(img):
    h, w = img.shape
    h2, w2 = (h + 1) // 2, (w + 1) // 2
    I = img.astype(np.int64)
    k = (1, 4, 6, 4, 1)
    rows = sum(k[j] * I[:, r101(2 * np.arange(w2) + j - 2, w)] for j in range(5))
    out = sum(k[j] * rows[r101(2 * np.arange(h2) + j - 2, h), :] for j in range(5))
    return ((out + 128) >> 8).astype(np.uint8)


def pyramid(img, max_level):
    levels = [np.ascontiguousarray(img, np.uint8)]
    for _ in range(max_level):
        levels.append(pyr_down(levels[-1]))
    return levels


# ---- step 2 ---------------------------------------------------------------------------------------------------------------------
def scharr(img):
    """(Ix, Iy) int64 at every pixel, neighbours through r101"""
    h, w = img.shape
    I = img.astype(np.int64)
    ym, yp = r101(np.arange(h) - 1, h), r101(np.arange(h) + 1, h)
    xm, xp = r101(np.arange(w) - 1, w), r101(np.arange(w) + 1, w)
    dx = I[:, xp] - I[:, xm]
    dy = I[yp, :] - I[ym, :]
    return 3 * dx[ym, :] + 10 * dx + 3 * dx[yp, :], 3 * dy[:, xm] + 10 * dy + 3 * dy[:, xp]


def _patch(m, ix, iy):
    """the 22 x 22 samples of map m at pixels (ix .. ix+21, iy .. iy+21), coordinates through r101"""
    h, w = m.shape
    return m[np.ix_(r101(iy + np.arange(WIN + 1), h), r101(ix + np.arange(WIN + 1), w))].astype(np.int64)


def _weights(a, b):
    one = F(1.0)
    w00 = int(np.rint(F(F(F(one - a) * F(one - b)) * F(16384.0))))
    w01 = int(np.rint(F(F(a * F(one - b)) * F(16384.0))))
    w10 = int(np.rint(F(F(F(one - a) * b) * F(16384.0))))
    return w00, w01, w10, 16384 - w00 - w01 - w10


def _interp(P, w, rnd, sh):
    w00, w01, w10, w11 = w
    return (w00 * P[:-1, :-1] + w01 * P[:-1, 1:] + w10 * P[1:, :-1] + w11 * P[1:, 1:] + rnd) >> sh


def _inside(fx, fy, w, h):
    """the bounds test of steps 3 and 5 on the floored f32 coordinates (false for NaN)"""
    return bool(fx >= F(-21.0) and fx < F(w) and fy >= F(-21.0) and fy < F(h))


def _i64f(v):
    return F(np.int64(v))


# ---- steps 3 - 6 ----------------------------------------------------------------------------------------------------------------
def track_point(cur, forw, derivs, pt, max_level):
    """One point through all levels.  Returns (x, y, status, codes[max_level+1], iters[max_level+1], causes): causes is a set of the
    events the branch-coverage test wants ("skip_upper", "skip0", "loweig0", ...)."""
    ptx, pty = F(pt[0]), F(pt[1])
    status = 1
    codes = np.zeros(max_level + 1, np.uint8); iters = np.zeros(max_level + 1, np.uint8)
    causes = set()
    nx = ny = F(0.0)
    with np.errstate(all="ignore"):
        for l in range(max_level, -1, -1):
            I, J = cur[l], forw[l]
            h, w = I.shape
            sc = F(1.0 / (1 << l))
            prx, pry = F(ptx * sc), F(pty * sc)
            if l == max_level:
                nx, ny = prx, pry
            else:
                nx, ny = F(nx * F(2.0)), F(ny * F(2.0))
            px, py = F(prx - HALF), F(pry - HALF)
            fx, fy = np.floor(px), np.floor(py)
            if not _inside(fx, fy, w, h):                     # step 3
                codes[l] = SKIP
                causes.add("skip0" if l == 0 else "skip_upper")
                if l == 0:
                    status = 0
                continue
            ix, iy = int(fx), int(fy)
            wts = _weights(F(px - fx), F(py - fy))
            Ix, Iy = derivs[l]
            Iw = _interp(_patch(I, ix, iy), wts, 256, 9)     # step 4
            Dx = _interp(_patch(Ix, ix, iy), wts, 8192, 14)
            Dy = _interp(_patch(Iy, ix, iy), wts, 8192, 14)
            A11 = F(_i64f((Dx * Dx).sum()) * S20); A12 = F(_i64f((Dx * Dy).sum()) * S20); A22 = F(_i64f((Dy * Dy).sum()) * S20)
            D = F(F(A11 * A22) - F(A12 * A12))
            dif = F(A11 - A22)
            root = np.sqrt(F(F(dif * dif) + F(F(F(4.0) * A12) * A12)))
            min_eig = F(F(F(A22 + A11) - root) / F(882.0))
            if min_eig < F(1e-4) or D < FLT_EPSILON:
                codes[l] = LOWEIG
                for name, hit in (("mineig", min_eig < F(1e-4)), ("det", D < FLT_EPSILON)):         # a flat patch meets both conditions
                    if hit:
                        causes.add(name + ("0" if l == 0 else "_upper"))
                if l == 0:
                    status = 0
                continue
            D = F(F(1.0) / D)
            nx, ny = F(nx - HALF), F(ny - HALF)                # step 5
            dpx = dpy = F(0.0)
            code, n_it = CAP, 0
            for j in range(MAX_ITERS):
                gx, gy = np.floor(nx), np.floor(ny)
                if not _inside(gx, gy, w, h):
                    code = OOB
                    if l == 0:
                        status = 0
                    break
                Jw = _interp(_patch(J, int(gx), int(gy)), _weights(F(nx - gx), F(ny - gy)), 256, 9)
                diff = Jw - Iw
                b1 = F(_i64f((diff * Dx).sum()) * S20); b2 = F(_i64f((diff * Dy).sum()) * S20)
                dx = F(F(F(A12 * b2) - F(A22 * b1)) * D); dy = F(F(F(A12 * b1) - F(A11 * b2)) * D)
                nx, ny = F(nx + dx), F(ny + dy)
                n_it = j + 1
                if F(F(dx * dx) + F(dy * dy)) <= F(1e-4):
                    code = EPS
                    break
                if j > 0 and abs(F(dx + dpx)) < F(0.01) and abs(F(dy + dpy)) < F(0.01):
                    nx, ny = F(nx - F(dx * F(0.5))), F(ny - F(dy * F(0.5)))
                    code = OSC
                    break
                dpx, dpy = dx, dy
            nx, ny = F(nx + HALF), F(ny + HALF)
            codes[l], iters[l] = code, n_it
            causes.add(CODE_NAMES[code])
        H, W = cur[0].shape
        rx, ry = np.rint(nx), np.rint(ny)                       # step 6 (false for NaN / infinity handled by the comparisons)
        if not (rx >= F(1.0) and rx < F(W - 1) and ry >= F(1.0) and ry < F(H - 1)):
            if status:
                causes.add("border")
            status = 0
    return nx, ny, status, codes, iters, causes


def track(cur, forw, pts, max_level):
    """cur, forw: pyramids (lists of uint8 arrays).  pts n x 2 float32.  Returns forw_xy (n x 2 f32), status (n u8), codes and iters
    (n x (max_level+1) u8, column l = level l) and the union of causes."""
    pts = np.asarray(pts, F).reshape(-1, 2)
    derivs = [scharr(m) for m in cur]
    n = len(pts)
    out = np.zeros((n, 2), F); st = np.zeros(n, np.uint8)
    codes = np.zeros((n, max_level + 1), np.uint8); iters = np.zeros((n, max_level + 1), np.uint8)
    causes = set()
    for i in range(n):
        x, y, s, c, it, ca = track_point(cur, forw, derivs, pts[i], max_level)
        out[i] = (x, y); st[i] = s; codes[i] = c; iters[i] = it; causes |= ca
    return out, st, codes, iters, causes


# ---- step 7 ---------------------------------------------------------------------------------------------------------------------
def set_mask(shape, tracks, min_dist):
    h, w = shape
    tracks = np.asarray(tracks, F).reshape(-1, 2)
    kept = np.zeros(len(tracks), np.uint8)
    mask = np.full((h, w), 255, np.uint8)
    yy, xx = np.mgrid[0:h, 0:w]
    pix = []
    with np.errstate(all="ignore"):
        for i, (x, y) in enumerate(tracks):
            rx, ry = np.rint(x), np.rint(y)
            if not (rx >= 0 and rx < F(w) and ry >= 0 and ry < F(h)):
                continue
            px, py = int(rx), int(ry)
            if any((px - qx) ** 2 + (py - qy) ** 2 <= min_dist * min_dist for qx, qy in pix):
                continue
            kept[i] = 1
            pix.append((px, py))
            mask[(xx - px) ** 2 + (yy - py) ** 2 <= min_dist * min_dist] = 0
    return kept, mask


# ---- step 8 ---------------------------------------------------------------------------------------------------------------------
def corner_response(img):
    h, w = img.shape
    I = img.astype(np.int64)
    ym, yp = r101(np.arange(h) - 1, h), r101(np.arange(h) + 1, h)
    xm, xp = r101(np.arange(w) - 1, w), r101(np.arange(w) + 1, w)
    dxc = I[:, xp] - I[:, xm]; dyc = I[yp, :] - I[ym, :]
    dx = dxc[ym, :] + 2 * dxc + dxc[yp, :]
    dy = dyc[:, xm] + 2 * dyc + dyc[:, xp]

    def box(m):
        r = m[ym, :] + m + m[yp, :]
        return r[:, xm] + r + r[:, xp]
    Sxx, Sxy, Syy = box(dx * dx), box(dx * dy), box(dy * dy)
    s = F(F(1.0) / F(12.0 * 255.0))
    s2 = F(s * s)
    a = (Sxx.astype(F) * s2) * F(0.5); b = Sxy.astype(F) * s2; c = (Syy.astype(F) * s2) * F(0.5)
    d = a - c
    return ((a + c) - np.sqrt(d * d + b * b)).astype(F)


# ---- steps 9, 10 ----------------------------------------------------------------------------------------------------------------
def candidates(eig, mask, quality):
    """(pixel indices in rank order, thr)"""
    h, w = eig.shape
    ok = (mask == 255) & (eig > 0)
    mx = eig[ok].max() if ok.any() else F(0.0)
    thr = F(mx * F(quality))
    t = np.where(eig > thr, eig, F(0.0))
    ys, xs = np.arange(h), np.arange(w)
    dil = t.copy()
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            dil = np.maximum(dil, t[np.ix_(r101(ys + dy, h), r101(xs + dx, w))])
    c = (eig > thr) & (eig == dil) & (mask == 255)
    c[0, :] = c[-1, :] = False; c[:, 0] = c[:, -1] = False
    idx = np.flatnonzero(c)
    order = np.lexsort((idx, -eig.ravel()[idx].astype(np.float64)))
    return idx[order], thr


def picks(ranked, width, min_dist, need):
    px = np.zeros(max(need, 1), np.int64); py = np.zeros(max(need, 1), np.int64)
    m = 0
    for p in ranked:
        if m >= need:
            break
        x, y = int(p % width), int(p // width)
        if m == 0 or ((px[:m] - x) ** 2 + (py[:m] - y) ** 2 >= min_dist * min_dist).all():
            px[m], py[m] = x, y
            m += 1
    return np.stack([px[:m], py[:m]], axis=1).astype(F)


def detect(img, tracks, min_dist, max_cnt, quality):
    """Returns kept (u8), new_xy (f32, pick order), eig (f32 map), mask (u8 map), n_candidates."""
    kept, mask = set_mask(img.shape, tracks, min_dist)
    eig = corner_response(img)
    ranked, _ = candidates(eig, mask, quality)
    need = max(0, max_cnt - int(kept.sum()))
    return kept, picks(ranked, img.shape[1], min_dist, need), eig, mask, len(ranked)


# ---- the resident chain the GPU tests replay ------------------------------------------------------------------------------------
class RefTracker:
    """push / track / detect with the row's image bookkeeping: the first image is both cur and forw"""

    def __init__(self, max_level):
        self.max_level = max_level
        self.cur = self.forw = None

    def push(self, img):
        p = pyramid(img, self.max_level)
        self.cur = p if self.forw is None else self.forw
        self.forw = p

    def track(self, pts):
        return track(self.cur, self.forw, pts, self.max_level)

    def detect(self, tracks, min_dist, max_cnt, quality=0.01):
        return detect(self.forw[0], tracks, min_dist, max_cnt, quality)
