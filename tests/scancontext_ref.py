"""numpy restatement of the arithmetic contract of include/vilsc.h (Scan Context place recognition), step by step as numbered there.

Every reduction of the contract is an explicit loop over the reduced index in ascending order (vectorised over everything else): there is
no np.sum / np.dot on them, whose order numpy does not define.  float32 arrays stay float32 through numpy's element-wise operations and
are rounded after each one, which is the unfused arithmetic the contract asks for.  Test infrastructure, not a timing baseline."""
import math

import numpy as np

NUM_RING, NUM_SECTOR = 20, 60
MODE_REFERENCE, MODE_EXHAUSTIVE = 0, 1
BIG = 10000000.0
F32, F64 = np.float32, np.float64


class Config:
    def __init__(self, lidar_height=2.0, max_radius=80.0, dist_thres=0.5, search_ratio=0.1, num_exclude_recent=5, num_candidates=3):
        self.lidar_height, self.max_radius, self.dist_thres, self.search_ratio = lidar_height, max_radius, dist_thres, search_ratio
        self.num_exclude_recent, self.num_candidates = num_exclude_recent, num_candidates

    @property
    def radius(self):
        return int(math.floor(0.5 * self.search_ratio * NUM_SECTOR + 0.5))         # C's round() of a non-negative value


# ---- step 1 ---------------------------------------------------------------------------------------------------------------------------
def xy2theta(x, y):
    x = np.asarray(x, F32); y = np.asarray(y, F32)
    k = 180.0 / math.pi
    with np.errstate(all="ignore"):
        b1 = k * np.arctan((y / x).astype(F64))
        b2 = 180.0 - k * np.arctan((y / (-x)).astype(F64))
        b3 = 180.0 + k * np.arctan((y / x).astype(F64))
        b4 = 360.0 - k * np.arctan(((-y) / x).astype(F64))
    return np.where((x >= 0) & (y >= 0), b1, np.where((x < 0) & (y >= 0), b2, np.where((x < 0) & (y < 0), b3, b4))).astype(F32)


def _ord(v):
    """order-preserving uint32 image of float32 values (-0 below +0)"""
    u = np.asarray(v, F32).view(np.uint32)
    return np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000)).astype(np.uint32)


def _ord_back(k):
    k = np.asarray(k, np.uint32)
    return np.where(k & np.uint32(0x80000000), k & np.uint32(0x7FFFFFFF), ~k).astype(np.uint32).view(F32)


def ring_sector(xyzi, cfg):
    """(keep mask, ring 1..20, sector 1..60, z') per point; ring / sector are meaningless where keep is False"""
    p = np.ascontiguousarray(xyzi, F32).reshape(-1, 4)
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    with np.errstate(all="ignore"):
        keep = np.isfinite(x) & np.isfinite(y) & ~((x == 0) & (y == 0))            # DEVIATION
        zp = (z.astype(F64) + cfg.lidar_height).astype(F32)
        rng = np.sqrt(x * x + y * y)                                               # float32 throughout
        theta = xy2theta(x, y)
        keep &= ~(rng.astype(F64) > cfg.max_radius)
        ring = np.ceil(np.where(keep, rng, 0).astype(F64) / cfg.max_radius * NUM_RING)
        sector = np.ceil(np.where(keep, theta, 0).astype(F64) / 360.0 * NUM_SECTOR)
    ring = np.clip(ring.astype(np.int64), 1, NUM_RING); sector = np.clip(sector.astype(np.int64), 1, NUM_SECTOR)
    return keep, ring, sector, zp


def make_descriptor(xyzi, cfg):
    keep, ring, sector, zp = ring_sector(xyzi, cfg)
    keep = keep & ~np.isnan(zp)                                                    # a NaN never wins desc < z
    table = np.zeros(NUM_RING * NUM_SECTOR, np.uint32)
    np.maximum.at(table, ((ring - 1) * NUM_SECTOR + (sector - 1))[keep], _ord(zp[keep]))
    d = _ord_back(np.maximum(table, _ord(F32(-1000.0)))).copy()
    d[d == F32(-1000.0)] = F32(0.0)
    return d.reshape(NUM_RING, NUM_SECTOR)


# ---- step 2 ---------------------------------------------------------------------------------------------------------------------------
def make_keys(desc):
    """(ring key float32 20, sector key float64 60, column norms float64 60)"""
    d = np.asarray(desc, F32).astype(F64)
    a = np.zeros(NUM_RING)
    for c in range(NUM_SECTOR):
        a = a + d[:, c]
    s = np.zeros(NUM_SECTOR); q = np.zeros(NUM_SECTOR)
    for r in range(NUM_RING):
        s = s + d[r]
        q = q + d[r] * d[r]
    with np.errstate(all="ignore"):
        return (a / 60.0).astype(F32), s / 20.0, np.sqrt(q)


# ---- step 3 ---------------------------------------------------------------------------------------------------------------------------
def candidates(ringkeys, query_key, n_search, k):
    """indices of the min(k, n_search) nearest ring keys of [0, n_search), ordered by (distance, index)"""
    keys = np.asarray(ringkeys, F32)[:n_search]
    acc = np.zeros(n_search, F32)
    with np.errstate(all="ignore"):
        for r in range(NUM_RING):
            d = F32(query_key[r]) - keys[:, r]
            acc = acc + d * d
    bits = np.where(np.isnan(acc), np.uint32(0x7FC00000), acc.view(np.uint32)).astype(np.uint64)
    order = np.argsort((bits << np.uint64(32)) | np.arange(n_search, dtype=np.uint64), kind="stable")
    return order[:min(k, n_search)].astype(np.int32)


# ---- step 4 ---------------------------------------------------------------------------------------------------------------------------
_J = np.arange(NUM_SECTOR)
_COL = (_J[None, :] - _J[:, None]) % NUM_SECTOR                                    # _COL[s, j] = (j - s) mod 60


def shift_distances(qd, qn, ed, en):
    """dist[e, s] for all 60 shifts: query (descriptor qd 20 x 60, norms qn) against entries ed (E x 20 x 60), en (E x 60)"""
    q = np.asarray(qd, F32).astype(F64); e = np.asarray(ed, F32).astype(F64)
    E = len(e)
    dot = np.zeros((E, NUM_SECTOR, NUM_SECTOR))                                    # [e, s, j]
    with np.errstate(all="ignore"):
        for r in range(NUM_RING):
            dot = dot + q[r][None, None, :] * e[:, r, :][:, _COL]
        total = np.zeros((E, NUM_SECTOR)); count = np.zeros((E, NUM_SECTOR))
        for j in range(NUM_SECTOR):
            nq = qn[j]; ne = en[:, _COL[:, j]]                                      # [e, s]
            skip = (ne == 0) | (nq == 0)
            total = np.where(skip, total, total + dot[:, :, j] / (nq * ne))
            count = count + ~skip
        return 1.0 - total / count


def fast_align(qv, ev):
    """fastAlignUsingVkey per entry: ev is E x 60"""
    E = len(ev)
    acc = np.zeros((E, NUM_SECTOR))                                                # [e, s]
    with np.errstate(all="ignore"):
        for j in range(NUM_SECTOR):
            d = qv[j] - ev[:, _COL[:, j]]
            acc = acc + d * d
        nrm = np.sqrt(acc)
    best = np.full(E, BIG); arg = np.zeros(E, np.int64)
    for s in range(NUM_SECTOR):
        m = nrm[:, s] < best
        arg = np.where(m, s, arg); best = np.where(m, nrm[:, s], best)
    return arg


def best_shift(dist, allowed):
    """strict < from 10000000 over the allowed shifts in ascending order: (min dist, argmin) per entry"""
    E = len(dist)
    best = np.full(E, BIG); arg = np.zeros(E, np.int64)
    for s in range(NUM_SECTOR):
        m = allowed[:, s] & (dist[:, s] < best)
        arg = np.where(m, s, arg); best = np.where(m, dist[:, s], best)
    return best, arg


# ---- the database and step 5 ------------------------------------------------------------------------------------------------------------
class Result:
    """min_dist, loop_id, nn_idx, nn_align, n_searched, yaw_diff_rad as in vsc_result; dist, shift, candidates as vsc_debug_read gives them"""


class Database:
    def __init__(self, cfg=None):
        self.cfg = cfg or Config()
        self.desc, self.ring, self.sect, self.norm = [], [], [], []

    def count(self):
        return len(self.desc)

    def push_descriptor(self, desc):
        d = np.array(desc, F32).reshape(NUM_RING, NUM_SECTOR)
        rk, sk, nm = make_keys(d)
        self.desc.append(d); self.ring.append(rk); self.sect.append(sk); self.norm.append(nm)
        return len(self.desc) - 1

    def push_scan(self, xyzi):
        return self.push_descriptor(make_descriptor(xyzi, self.cfg))

    def detect(self, mode=MODE_REFERENCE, n_search=-1):
        cfg = self.cfg
        out = Result()
        out.dist, out.shift, out.candidates = np.zeros(0), np.zeros(0, np.int32), np.zeros(0, np.int32)
        out.min_dist, out.loop_id, out.nn_idx, out.nn_align, out.n_searched, out.yaw_diff_rad = BIG, -1, 0, 0, 0, F32(0.0)
        if self.count() < cfg.num_exclude_recent + 1:
            return out
        if n_search < 0:
            n_search = self.count() - cfg.num_exclude_recent
        assert 1 <= n_search <= self.count()
        q = self.count() - 1
        if mode == MODE_REFERENCE:
            visit = candidates(np.array(self.ring), self.ring[q], n_search, cfg.num_candidates)
        else:
            visit = np.arange(n_search, dtype=np.int32)
        dist = shift_distances(self.desc[q], self.norm[q], np.array([self.desc[i] for i in visit]), np.array([self.norm[i] for i in visit]))
        if mode == MODE_REFERENCE:
            a = fast_align(self.sect[q], np.array([self.sect[i] for i in visit]))
            dd = np.abs(_J[None, :] - a[:, None])
            allowed = np.minimum(dd, NUM_SECTOR - dd) <= cfg.radius
        else:
            allowed = np.ones((len(visit), NUM_SECTOR), bool)
        best, arg = best_shift(dist, allowed)
        for slot in range(len(visit)):                                             # step 5
            if best[slot] < out.min_dist:
                out.min_dist, out.nn_align, out.nn_idx = float(best[slot]), int(arg[slot]), int(visit[slot])
        if out.min_dist < cfg.dist_thres:
            out.loop_id = out.nn_idx
        out.yaw_diff_rad = F32(F64(F32(out.nn_align * 6.0)) * math.pi / 180.0)
        out.n_searched = n_search
        out.dist, out.shift, out.candidates = best, arg.astype(np.int32), visit
        out.all_shifts = dist
        return out
