"""numpy / float32 restatement of include/vilscan.h (steps 1-6 of its header), written from that definition and sharing no code with the
library.  Every float32 array operation below is one IEEE float32 operation per element, in the order of the reference's source
(numpy does not contract a * b + c); comparisons against the reference's double literals are done in float64.  Serial over rings,
subregions and picks.  Test infrastructure: not a timing baseline."""
import numpy as np

F = np.float32


class Config:
    def __init__(self, num_rings=16, lower=-15.0, upper=15.0, S=8, C=5, th=1.0, max_sharp=3, max_less=30, max_flat=4, leaf=0.2):
        self.num_rings, self.lower, self.upper, self.S, self.C = num_rings, F(lower), F(upper), S, C
        self.th, self.max_sharp, self.max_less, self.max_flat, self.leaf = F(th), max_sharp, max_less, max_flat, F(leaf)


class Result:
    pass


def ring_ids(xyzi, cfg):
    """Step 1: ring of every raw point, -1 = dropped."""
    p = np.ascontiguousarray(xyzi, F).reshape(-1, 4)
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    ids = np.full(len(p), -1, np.int64)
    fin = np.isfinite(x) & np.isfinite(y) & np.isfinite(z)
    with np.errstate(all="ignore"):
        dis = np.sqrt(x * x + y * y)                                  # float32
        ele = np.arctan2(z, dis)                                      # float32 (atan2f)
        factor = np.float64(cfg.num_rings - 1) / (np.float64(cfg.upper) - np.float64(cfg.lower))
        v = (ele.astype(np.float64) * 180.0 / np.pi - np.float64(cfg.lower)) * factor + 0.5
    ok = fin & (v > -1.0) & (v < cfg.num_rings)
    ids[ok] = np.trunc(v[ok]).astype(np.int64)                        # int(): truncation towards zero
    return ids


def _sqdiff(a, b):
    dx = a[..., 0] - b[..., 0]; dy = a[..., 1] - b[..., 1]; dz = a[..., 2] - b[..., 2]
    return dx * dx + dy * dy + dz * dz


def _sqdiff_w(a, b, wb):
    dx = a[..., 0] - b[..., 0] * wb; dy = a[..., 1] - b[..., 1] * wb; dz = a[..., 2] - b[..., 2] * wb
    return dx * dx + dy * dy + dz * dz


def _sqnorm(a):
    return a[..., 0] * a[..., 0] + a[..., 1] * a[..., 1] + a[..., 2] * a[..., 2]


def prepare_ring(ring, C):
    """Step 2: PrepareRing.  Returns the mask (uint8).  The decision at i reads points i - 1, i, i + 1 only and the writes only set
    entries, so the quantities are computed for all i at once and the writes applied afterwards."""
    n = len(ring)
    mask = np.zeros(n, np.uint8)
    i = np.arange(C, n - C)
    pp, pc, pn = ring[i - 1], ring[i], ring[i + 1]
    with np.errstate(all="ignore"):
        diff_next2 = _sqdiff(pc, pn)
        far = diff_next2.astype(np.float64) > 0.1
        depth = np.sqrt(_sqnorm(pc)); depth_next = np.sqrt(_sqnorm(pn))
        closer = depth > depth_next
        wd_a = np.sqrt(_sqdiff_w(pn, pc, depth_next / depth)) / depth_next
        wd_b = np.sqrt(_sqdiff_w(pc, pn, depth / depth_next)) / depth
        back = far & closer & (wd_a.astype(np.float64) < 0.1)
        fwd = far & ~closer & (wd_b.astype(np.float64) < 0.1)
        diff_prev2 = _sqdiff(pc, pp); dis2 = _sqnorm(pc)
        lim = 0.0002 * dis2.astype(np.float64)
        own = ~back & ~fwd & (diff_next2.astype(np.float64) > lim) & (diff_prev2.astype(np.float64) > lim)
    for k in i[back]:
        mask[k - C:k + 1] = 1
    for k in i[fwd]:
        mask[k + 1:min(k + C + 2, n)] = 1                                 # the reference writes one past the end when i = n - C - 1: clamped
    mask[i[own]] = 1
    assert diff_next2.dtype == F and wd_a.dtype == F and dis2.dtype == F
    return mask


def curvature_and_vote(ring, sp, ep, C):
    """Step 3 for the indices sp..ep: (curvature float32, vote int)."""
    idx = np.arange(sp, ep + 1)
    with np.errstate(all="ignore"):
        nn = F(-2 * C)
        d = [nn * ring[idx, a] for a in range(3)]
        vote = np.zeros(len(idx), np.int64)
        for k in range(1, C + 1):
            for a in range(3):
                d[a] = d[a] + (ring[idx + k, a] + ring[idx - k, a])
            ra = ring[idx + k, 3] / ring[idx, 3]; rb = ring[idx - k, 3] / ring[idx, 3]
            vote += ((ra >= 1) & (ra < 2)).astype(np.int64) + ((rb >= 1) & (rb < 2)).astype(np.int64)
        curv = d[0] * d[0] + d[1] * d[1] + d[2] * d[2]
    assert curv.dtype == F
    return curv, vote


def _mask_picked(ring, mask, i, C):
    mask[i] = 1
    for k in range(1, C + 1):
        if np.float64(_sqdiff(ring[i + k], ring[i + k - 1])) > 0.05:
            break
        mask[i + k] = 1
    for k in range(1, C + 1):
        if np.float64(_sqdiff(ring[i - k], ring[i - k + 1])) > 0.05:
            break
        mask[i - k] = 1


def voxel_filter(pts, leaf):
    """Step 6: exact voxel filter, cells in order of first occurrence, fp64 mean rounded once."""
    if len(pts) == 0:
        return np.zeros((0, 4), F)
    inv = F(1.0) / F(leaf)
    cells = np.floor(pts[:, :3] * inv).astype(np.int64)
    order, sums, cnt = {}, [], []
    for q in range(len(pts)):
        key = (int(cells[q, 0]), int(cells[q, 1]), int(cells[q, 2]))
        k = order.get(key)
        if k is None:
            k = order[key] = len(sums); sums.append(np.zeros(4, np.float64)); cnt.append(0)
        sums[k] = sums[k] + pts[q].astype(np.float64); cnt[k] += 1
    return np.stack([(s / np.float64(c)).astype(F) for s, c in zip(sums, cnt)])


def extract(xyzi, cfg=None):
    cfg = cfg or Config()
    p = np.ascontiguousarray(xyzi, F).reshape(-1, 4)
    ids = ring_ids(p, cfg)
    C, S = cfg.C, cfg.S
    th_hi = cfg.th / F(2); th_lo = cfg.th / F(10)
    out = Result()
    rings = [p[ids == r] for r in range(cfg.num_rings)]               # boolean indexing keeps the arrival order
    out.cloud = np.concatenate(rings) if len(p) else np.zeros((0, 4), F)
    cnts = np.array([len(r) for r in rings], np.int64)
    out.ring_table = np.stack([np.cumsum(cnts) - cnts, cnts], axis=1).astype(np.int32)
    labels = np.zeros(len(out.cloud), np.int8)
    sharp, less, flat, lf_ds = [], [], [], []
    out.n_less_flat_raw = 0
    out.masks = []
    for r, ring in enumerate(rings):
        n = len(ring); start = int(out.ring_table[r, 0])
        if n <= 2 * C + 1:
            out.masks.append(np.zeros(n, np.uint8))
            continue
        mask = prepare_ring(ring, C)
        lab = labels[start:start + n]
        lf = []
        for j in range(S):
            sp = (C * (S - j) + (n - C) * j) // S
            ep = (C * (S - 1 - j) + (n - C) * (j + 1)) // S - 1
            if ep <= sp:
                continue
            curv, vote = curvature_and_vote(ring, sp, ep, C)
            m1 = (curv > th_hi) & (vote > 4)
            m2 = ~m1 & (curv < th_lo) & (vote < 5)
            mask[sp:ep + 1] |= (m1 | m2).astype(np.uint8)
            order = sorted(range(sp, ep + 1), key=lambda i: (curv[i - sp], i))     # the total order of pair<float, size_t>
            picked = 0
            for i in reversed(order):
                if picked >= cfg.max_less:
                    break
                if mask[i] == 0 and curv[i - sp] > th_hi:
                    picked += 1
                    if picked <= cfg.max_sharp:
                        lab[i] = 2; sharp.append(ring[i])
                    else:
                        lab[i] = 1
                    less.append(ring[i])
                    _mask_picked(ring, mask, i, C)
            picked = 0
            for i in order:
                if picked >= cfg.max_flat:
                    break
                if mask[i] == 0 and curv[i - sp] < th_lo:
                    picked += 1
                    lab[i] = -1; flat.append(ring[i])
                    _mask_picked(ring, mask, i, C)
            lf.extend(i for i in range(sp, ep + 1) if lab[i] <= 0)
        out.masks.append(mask)
        out.n_less_flat_raw += len(lf)
        if lf:
            lf_ds.append(voxel_filter(ring[lf], cfg.leaf))
    st = lambda l: np.stack(l).astype(F) if l else np.zeros((0, 4), F)
    out.labels = labels
    out.corner_sharp, out.corner_less_sharp, out.surf_flat = st(sharp), st(less), st(flat)
    out.surf_less_flat = np.concatenate(lf_ds) if lf_ds else np.zeros((0, 4), F)
    return out
