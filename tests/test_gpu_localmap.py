"""GPU checks of include/villmap.h (lidar_mapping's local cube map as one resident call), through the C-ABI.  Everything is compared on
raw bytes: with the sequential restatement tests/localmap_ref.py for the bookkeeping, with vcloud_filter for every filtered cloud, and
with vmap_set_map + vmap_align for the alignment.  Only the matrix of step 6 has a tolerance: it is the device's quaternion -> R and is
held to 16 x the float64 floor against exact rational arithmetic."""
import hashlib
import os
import subprocess
import sys
from fractions import Fraction

import numpy as np
import pytest

import cloud_ref
import localmap_ref as R
from mvil_fusion_amd import cloud, lib, localmap, mapreg

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
I0 = np.array([0.0, 0.0, 0.0, 1.0])
SMALL = dict(max_scan_points=256, max_map_points=4096, publish_first_frame=3, publish_frames=5, publish_distance=1000.0)
CHAIN = dict(max_scan_points=4096, max_map_points=1 << 16, publish_first_frame=4, publish_frames=8)
REF_KEYS = set(R.DEFAULTS)
POPULATIONS = (0, 1, 63, 64, 65, 257, 5000)      # wave edges, more than a workgroup's width, and more than four waves' first steps (there is one path for all)
FLOOR_FACTOR = 16.0


def raw_bytes(a):
    return np.ascontiguousarray(a).view(np.uint8)


def same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(raw_bytes(a), raw_bytes(b))


def index(i, j, k):
    return i + R.W * j + R.W * R.H * k


def ref_of(cfg, make=R.LocalMapRef):
    return make(**{k: v for k, v in cfg.items() if k in REF_KEYS})


@pytest.fixture(scope="module")
def so():
    return lib.load_vilsolve()


@pytest.fixture(scope="module")
def solver():
    be = lib.open_vilsolve(device=0)
    yield be
    be.close()


@pytest.fixture(scope="module")
def small(so):
    m = localmap.LocalMap(so, **SMALL)
    yield m
    m.close()


@pytest.fixture(scope="module")
def filt(so):
    f = cloud.DepthCloud(so, max_scan_points=8192, max_scans=1)
    yield f
    f.close()


def device_cubes(m):
    return [m.cubes(0), m.cubes(1)]


def cubes_digest(m):
    h = hashlib.sha256()
    for cls in range(2):
        for e, c in enumerate(m.cubes(cls)):
            if len(c):
                h.update(np.asarray([cls, e, len(c)], np.int64).tobytes()); h.update(c.tobytes())
    return h.hexdigest()


def compare(m, ref, s, res, label):
    """The device after a push against the restatement after the same push."""
    assert localmap.summary_counts(s) == res.counts(), (label, localmap.summary_counts(s), res.counts())
    assert np.array(s.q_w_curr).tobytes() == res.q.tobytes() and np.array(s.t_w_curr).tobytes() == res.t.tobytes(), label
    for stage, want in ((localmap.DBG_CORNER_STACK, res.stack[0]), (localmap.DBG_SURF_STACK, res.stack[1]), (localmap.DBG_CORNER_FROM_MAP, res.from_map[0]),
                        (localmap.DBG_SURF_FROM_MAP, res.from_map[1])):
        assert same(m.debug_read(stage), want), (label, "stage", stage)
    for cls in range(2):
        for e, c in enumerate(m.cubes(cls)):
            assert same(c, ref.cube(cls, e)), (label, "cube", cls, e, len(c), len(ref.cube(cls, e)))
    if res.published is not None:
        assert same(m.read_published(localmap.FRAME_WORLD), res.published[0]) and same(m.read_published(localmap.FRAME_SENSOR), res.published[1]), label


# ---- bookkeeping without alignment -------------------------------------------------------------------------------------------------------
COORDS = np.asarray((10.0, np.nextafter(F(10.0), F(0.0)), 0.0, -0.0, -1e-30, -10.0, -10.000001, -20.0), F)


def quirk_and_teleport_chain():
    """[(corner, surf, q, t)]: the quirk coordinates placed through three exactly representable poses, then teleports that force every
    shift direction and a double shift.  At most 8 corner and 6 surf points per scan and a publication every six frames: never more than
    50 surf points in the map, so the gate of step 5 stays shut and the pose is the guess."""
    world = np.array([[v, F(0.5 + 0.3 * n), F(0.5) * v, 7.0 + n] for n, v in enumerate(COORDS)], F)
    chain = [(world, R.empty(), I0, np.zeros(3))]
    t1 = np.array([20.0, -10.0, 5.0])
    p1 = world.copy(); p1[:, :3] = (world[:, :3].astype(np.float64) - t1).astype(F)
    chain.append((p1, R.empty(), I0, t1))
    t2 = np.array([-10.0, 10.0, -5.0])                                             # yaw of 180 degrees, an exact quaternion: world = (-x, -y, z) + t
    p2 = world.copy(); p2[:, :3] = ((world[:, :3].astype(np.float64) - t2) * [-1.0, -1.0, 1.0]).astype(F)
    chain.append((p2, R.empty(), np.array([0.0, 0.0, 1.0, 0.0]), t2))
    rng = np.random.default_rng(2)
    for t in ([-25.0, 0.0, 0.0], [-25.0, -25.0, 0.0], [-25.0, -25.0, -2.5], [35.0, -25.0, -2.5], [35.0, 45.0, 7.5], [-45.0, 45.0, 7.5], [-45.0, 45.0, -12.5], [0.0, -55.0, 0.0],
              [1.0, -55.0, 0.0]):
        clouds = [np.concatenate([rng.uniform(-1.0, 1.0, (n, 3)) * [26.0, 26.0, 8.0], rng.uniform(0.0, 9.0, (n, 1))], axis=1).astype(F) for n in (8, 6)]
        chain.append((clouds[0], clouds[1], R.yaw_quat(0.25 * len(chain)), np.array(t)))
    return chain


def test_bookkeeping_matches_the_restatement_without_alignment(small, solver):
    small.reset()
    ref = ref_of(SMALL)
    seen = set(); published = 0
    for k, (corner, surf, q, t) in enumerate(quirk_and_teleport_chain()):
        s = small.push_scan(solver.ctx, corner, surf, q, t)
        res = ref.push(corner, surf, q, t)
        assert s.aligned == 0 and res.aligned == 0
        compare(small, ref, s, res, "push %d" % k)
        assert same(small.debug_read(localmap.DBG_MATRIX), R.matrix_of(res.q, res.t))              # the host's quat_to_R of the guess
        for ax in range(3):
            if res.shift[ax]:
                seen.add((ax, int(np.sign(res.shift[ax])), abs(res.shift[ax]) > 1))
        published += s.published
        if k == 0:                                                                                 # the table of the issue, in float32
            occ = {e: len(c) for e, c in enumerate(small.cubes(0)) if len(c)}
            assert occ == {index(6, 5, 4): 1, index(5, 5, 3): 3, index(4, 5, 2): 1, index(3, 5, 1): 2, index(2, 5, 0): 1}, occ
    assert {(ax, sg) for ax, sg, _ in seen} == {(ax, sg) for ax in range(3) for sg in (1, -1)}, seen
    assert any(multi for _, _, multi in seen) and published >= 2


def test_an_invalid_cube_keeps_raw_points_until_it_becomes_valid(small, solver):
    small.reset()
    ref = ref_of(SMALL)
    far = np.array([[31.01, 1.0, 1.0, 1.0], [31.31, 1.0, 1.0, 2.0]], F)            # two voxels of 0.2, three cubes from the centre
    for k in range(2):
        s = small.push_scan(solver.ctx, far, R.empty(), I0, np.zeros(3)); res = ref.push(far, R.empty(), I0, np.zeros(3))
        compare(small, ref, s, res, "far %d" % k)
    assert small.read_cube(0, index(8, 5, 3))[:, 3].tolist() == [1.0, 2.0, 1.0, 2.0]               # unfiltered, in arrival order
    t = np.array([11.0, 0.0, 0.0])
    s = small.push_scan(solver.ctx, R.empty(), R.empty(), I0, t); res = ref.push(R.empty(), R.empty(), I0, t)
    compare(small, ref, s, res, "valid")
    assert small.read_cube(0, index(8, 5, 3))[:, 3].tolist() == [1.0, 2.0]                        # filtered once


# ---- the segmented filter alone ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hist", (1, 64, 512))
def test_segmented_filter_equals_filter_a_of_every_cube_alone(so, solver, filt, hist):
    """Cubes loaded raw through the test hook; one push with empty scans refilters the 75 valid ones.  make_cloud(kind, n) is a prefix of
    make_cloud(kind, m): all cubes of a kind hold points with IDENTICAL voxels and table entries, so an entry shared between two
    workgroups would show in either."""
    m = localmap.LocalMap(so, hist_size=hist, line_res=cloud_ref.LEAF, max_scan_points=64, max_map_points=1 << 15)
    valid = R.valid_cubes((5, 5, 3))
    try:
        for kind in ("alternating", "one_voxel"):
            m.reset()
            m.profile_enable(True); m.profile_read()
            raw = {}
            for slot, n in enumerate(POPULATIONS):
                raw[(0, valid[3 * slot])] = cloud_ref.make_cloud(kind, n)
            raw[(0, valid[40])] = cloud_ref.make_cloud(kind, 257)[::-1].copy()                     # the same voxels, met in the other order
            raw[(1, valid[41])] = cloud_ref.make_cloud("random", 300)                              # the surf class and its leaf
            raw[(0, index(0, 0, 0))] = cloud_ref.make_cloud(kind, 65)                              # not valid: stays raw
            for (cls, e), pts in raw.items():
                m.debug_write_cube(cls, e, pts)
            s = m.push_scan(solver.ctx, R.empty(), R.empty(), I0, np.zeros(3))
            assert s.n_corner_from_map == sum(len(p) for (cls, e), p in raw.items() if cls == 0 and e in valid)
            for (cls, e), pts in raw.items():
                got = m.read_cube(cls, e)
                if e not in valid:
                    assert same(got, pts)
                    continue
                leaf = m.cfg.plane_res if cls else m.cfg.line_res
                assert same(got, filt.filter(pts, leaf, hist)), (kind, hist, cls, e, len(pts))
                assert same(got, cloud_ref.filter_seq(pts, leaf, hist).out), (kind, hist, cls, e, len(pts))
            assert s.n_corner_map == sum(len(m.read_cube(0, e)) for (cls, e) in raw if cls == 0)
        # a one-cube map and a 75-cube map: the same launches
        m.reset(); m.profile_read()
        m.debug_write_cube(0, valid[0], cloud_ref.make_cloud("random", 100))
        m.push_scan(solver.ctx, cloud_ref.make_cloud("random", 20), cloud_ref.make_cloud("random", 20), I0, np.zeros(3))
        one = m.profile_read()
        m.reset()
        for e in valid:
            m.debug_write_cube(0, e, cloud_ref.make_cloud("random", 100)); m.debug_write_cube(1, e, cloud_ref.make_cloud("lidar", 200))
        m.push_scan(solver.ctx, cloud_ref.make_cloud("random", 20), cloud_ref.make_cloud("random", 20), I0, np.zeros(3))
        full = m.profile_read()
        m.profile_enable(False)
        assert {k: v[0] for k, v in one.items()} == {k: v[0] for k, v in full.items()}, (one, full)
        assert one["k_lmap_refilter"][0] == 1 and one["k_lmap_append"][0] == 1 and one["k_lmap_publish"][0] == 0
    finally:
        m.close()


# ---- the chain with alignment ------------------------------------------------------------------------------------------------------------
def exact_matrix_error(M, q):
    """max |M[:, :3] - R(q)| with R(q) in exact rational arithmetic from the doubles of q, and the same for the float64 restatement (the floor)."""
    x, y, z, w = (Fraction(float(c)) for c in q)
    Rx = [[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)], [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
          [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]]
    Rn = R.quat_to_R(q)
    err = max(abs(float(Fraction(float(M[r, c])) - Rx[r][c])) for r in range(3) for c in range(3))
    floor = max(abs(float(Fraction(float(Rn[r, c])) - Rx[r][c])) for r in range(3) for c in range(3))
    return err, floor


def run_chain(m, solver, reg=None, filt=None, ref=None, check=None):
    """The room walk into m; with reg / filt / ref also through the chain of public calls, compared after every push.  Returns a digest."""
    m.reset()
    h = hashlib.sha256()
    facts = dict(aligned=0, published=0, centres=set(), worst=0.0, floor=0.0)
    for k, (corner, surf, q, t) in enumerate(R.room_chain()):
        s = m.push_scan(solver.ctx, corner, surf, q, t)
        a = s.align
        h.update(repr(localmap.summary_counts(s)).encode()); h.update(np.array(s.q_w_curr).tobytes()); h.update(np.array(s.t_w_curr).tobytes())
        h.update(repr((a.rounds, a.n_edge, a.n_plane, a.iterations)).encode()); h.update(np.array([a.initial_cost, a.final_cost]).tobytes())
        h.update(cubes_digest(m).encode())
        if s.published:
            h.update(m.read_published(localmap.FRAME_WORLD).tobytes()); h.update(m.read_published(localmap.FRAME_SENSOR).tobytes())
        if ref is None:
            continue
        M = m.debug_read(localmap.DBG_MATRIX)
        sums = []

        def public_align(fc, fs, sc, ss, qg, tg, gate):
            reg.set_map(fc, fs)
            if not gate:
                return qg, tg, None
            q2, t2, sm = reg.align(solver.ctx, sc, ss, qg, tg)
            sums.append(sm)
            return q2, t2, sm

        res = ref.push(corner, surf, q, t, align=public_align, matrix=M)
        compare(m, ref, s, res, "chain %d" % k)
        assert same(filt.filter(corner, m.cfg.line_res, m.cfg.hist_size), res.stack[0]) and same(filt.filter(surf, m.cfg.plane_res, m.cfg.hist_size), res.stack[1])
        for (cls, e), pts in res.raw.items():                                                      # every valid cube: vcloud_filter of the cube alone
            assert same(filt.filter(pts, m.cfg.plane_res if cls else m.cfg.line_res, m.cfg.hist_size), res.filtered[(cls, e)]), (k, cls, e)
        if sums:
            sm = sums[0]
            assert (a.rounds, a.n_edge, a.n_plane, a.iterations) == (sm.rounds, sm.n_edge, sm.n_plane, sm.iterations), k
            assert np.array([a.initial_cost, a.final_cost]).tobytes() == np.array([sm.initial_cost, sm.final_cost]).tobytes(), k
        else:
            assert (a.rounds, a.n_edge, a.n_plane, a.iterations, a.initial_cost, a.final_cost) == (0, 0, 0, 0, 0.0, 0.0)
        assert np.array_equal(M[:, 3], np.array(s.t_w_curr))                                       # the translation is the pose's, bit for bit
        err, floor = exact_matrix_error(M, s.q_w_curr)
        facts["worst"] = max(facts["worst"], err); facts["floor"] = max(facts["floor"], floor)
        facts["aligned"] += s.aligned; facts["published"] += s.published
        facts["centres"].add(res.valid[0])
    if check is not None:
        check.update(facts)
    return h.hexdigest()


@pytest.fixture(scope="module")
def chain_map(so):
    m = localmap.LocalMap(so, **CHAIN)
    yield m
    m.close()


def test_chain_equals_the_chain_of_public_calls(so, solver, chain_map, filt):
    reg = mapreg.MapReg(so)
    facts = {}
    try:
        run_chain(chain_map, solver, reg=reg, filt=filt, ref=ref_of(CHAIN), check=facts)
    finally:
        reg.close()
    assert facts["aligned"] >= 5 and facts["published"] >= 1 and len(facts["centres"]) >= 2, facts        # the gate, a publication, a cube boundary
    ratio = facts["worst"] / facts["floor"] if facts["floor"] > 0 else (0.0 if facts["worst"] == 0 else float("inf"))
    print("matrix of step 6 against exact quat -> R: worst |M - R| %.3e, float64 floor %.3e, ratio %.2f" % (facts["worst"], facts["floor"], ratio))
    assert facts["worst"] <= FLOOR_FACTOR * facts["floor"], (facts, ratio)


CHILD = r"""
import sys
sys.path.insert(0, %r); sys.path.insert(0, %r)
import __graft_entry__ as graft
graft.load_package()
import test_gpu_localmap as T
from mvil_fusion_amd import lib, localmap
be = lib.open_vilsolve(device=0)
m = localmap.LocalMap(lib.load_vilsolve(), **T.CHAIN)
print("digest", T.run_chain(m, be))
m.close(); be.close()
"""


def test_reproducible_across_contexts_and_processes(so, solver, chain_map):
    a = run_chain(chain_map, solver)
    assert run_chain(chain_map, solver) == a
    other = localmap.LocalMap(so, **{**CHAIN, "max_scan_points": 5000, "max_map_points": 70000})   # another context, other capacities
    try:
        assert run_chain(other, solver) == a
    finally:
        other.close()
    code = CHILD % (ROOT, os.path.join(ROOT, "tests"))
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=120)     # a fresh child process, never an exec
    assert out.returncode == 0, out.stderr[-2000:]
    assert out.stdout.split()[-2:] == ["digest", a]


# ---- errors ------------------------------------------------------------------------------------------------------------------------------
def test_refused_calls_leave_the_cubes_alone(small, solver):
    small.reset()
    rng = np.random.default_rng(9)
    cl = lambda n: np.concatenate([rng.uniform(-20.0, 20.0, (n, 3)), np.ones((n, 1))], axis=1).astype(F)      # noqa: E731
    small.push_scan(solver.ctx, cl(8), cl(6), I0, np.zeros(3))
    small.debug_write_cube(0, index(5, 5, 3), cl(3900))
    before = cubes_digest(small)
    for name, args, status in (("oversize", (cl(257), cl(6), I0, np.zeros(3)), localmap.ERR_INVALID_ARGUMENT),
                               ("capacity", (cl(200), cl(6), I0, np.zeros(3)), localmap.ERR_CAPACITY),
                               ("nan pose", (cl(8), cl(6), I0, np.array([0.0, np.nan, 0.0])), localmap.ERR_INVALID_ARGUMENT),
                               ("nan quaternion", (cl(8), cl(6), np.array([0.0, 0.0, np.nan, 1.0]), np.zeros(3)), localmap.ERR_INVALID_ARGUMENT),
                               ("zero quaternion", (cl(8), cl(6), np.zeros(4), np.zeros(3)), localmap.ERR_INVALID_ARGUMENT)):
        with pytest.raises(localmap.LocalMapError) as e:
            small.push_scan(solver.ctx, *args)
        assert e.value.status == status, name
        assert cubes_digest(small) == before, name
    s = small.push_scan(solver.ctx, cl(8), cl(6), I0, np.zeros(3))                                  # and the context goes on
    assert s.frame_count == 2 and cubes_digest(small) != before
