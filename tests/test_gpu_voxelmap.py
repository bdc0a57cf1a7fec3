"""The device builder of VGICP's target voxel map (include/vilvgicp_voxel.h) against the host builder and against the sequential restatement
(tests/voxelmap_ref.py).  Nothing in the contract is transcendental: "equal" is raw bytes of vgicp_read_voxels against BOTH, and raw bytes of
everything computed from the map (linearisation, alignment, loop verification) between the builders.  There is no tolerance anywhere."""
import ctypes as C

import numpy as np
import pytest

import voxelmap_ref as ref
from mvil_fusion_amd import lib, loopverify as lv, vgicp

pytestmark = pytest.mark.gpu

F = np.float32
MODES = (vgicp.DIRECT1, vgicp.DIRECT7, vgicp.DIRECT27)
T_SMALL = np.eye(4)
T_SMALL[:3, :3] = vgicp._rot(0.004, -0.003, 0.006); T_SMALL[:3, 3] = (0.03, -0.02, 0.01)


def raw(a):
    return np.ascontiguousarray(a).view(np.uint8)


def same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(raw(a), raw(b))


def struct_bytes(s):
    return bytes(C.string_at(C.addressof(s), C.sizeof(s)))


@pytest.fixture(scope="module")
def so():
    return lib.load_vilsolve()


@pytest.fixture(scope="module")
def host(so):
    g = vgicp.Vgicp(so)
    yield g
    g.close()


@pytest.fixture(scope="module")
def dev(so):
    g = vgicp.Vgicp(so)
    g.set_voxel_builder(vgicp.BUILD_DEVICE)
    yield g
    g.close()


@pytest.fixture(scope="module")
def pairs():
    """The synthetic scan pairs, made once: 2 400 points (exhaustive neighbour search) and 14 400 points (grid search)."""
    return {n: vgicp.make_pair(0, rings=16, az=n // 16) for n in (2400, 14400)}


def check_map(host, dev, xyz, cov, res=ref.RES):
    """Both builders on the same cloud; the device builder's map equals the host builder's and the restatement's.  Returns the map."""
    host.set_target(xyz, cov, res); dev.set_target(xyz, cov, res)
    mh, md = host.read_voxels(), dev.read_voxels()
    want = ref.build(xyz, cov, res)
    assert len(md["keys"]) == len(want["keys"]) == len(mh["keys"])
    for f in ("keys", "num", "mean", "cov", "wsq"):
        assert same(md[f], want[f]), "device builder against the restatement: " + f
        assert same(mh[f], want[f]), "host builder against the restatement: " + f
        assert same(md[f], mh[f]), "device builder against the host builder: " + f
    return md


def lin_bytes(g, T, mode):
    err, H, b, nc = g.linearize(T, mode)
    return np.float64(err).tobytes() + raw(H).tobytes() + raw(b).tobytes() + np.int32(nc).tobytes(), nc


def check_linearize(host, dev, transforms=(np.eye(4), T_SMALL)):
    hit = 0
    for mode in MODES:
        for T in transforms:
            a, nc = lin_bytes(host, T, mode); b, _ = lin_bytes(dev, T, mode)
            assert a == b, (mode, nc)
            hit += nc
    assert hit > 0                                                          # the comparison is of correspondences, not of two empty sums


# ---- 1. tiny clouds ---------------------------------------------------------------------------------------------------------------
def test_tiny_clouds(host, dev):
    rng = np.random.default_rng(1)
    one = np.array([[0.3, -1.2, 2.6]], F)
    m = check_map(host, dev, one, ref.random_cov(rng, 1))
    assert m["num"].tolist() == [1] and m["wsq"].tolist() == [1.0]
    two = np.array([[0.30, 0.30, 0.30], [0.40, 0.45, 0.35]], F)
    m = check_map(host, dev, two, ref.random_cov(rng, 2))
    assert m["num"].tolist() == [2]
    pts = ref.boundary_cloud()
    check_map(host, dev, pts, ref.random_cov(rng, len(pts)))
    check_map(host, dev, pts, ref.random_cov(rng, len(pts)), 0.25)          # another resolution: other boundaries, no special case
    z = ref.zero_cloud()
    cov = np.zeros((8, 9)); cov[:, ::2] = -0.0
    for k in (1, 8):
        m = check_map(host, dev, z[:k], cov[:k])
        assert not np.signbit(m["mean"]).any() and not np.signbit(m["cov"]).any()


# ---- 2. the order of the sums -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_total", [600, 257, 1025])
def test_order_fixture(host, dev, n_total):
    xyz, cov, which = ref.order_fixture(n_total)
    assert ref.order_matters(xyz, cov, which, 0)                             # (asserted on the CPU too: tests/test_voxelmap_ref.py)
    m = check_map(host, dev, xyz, cov)
    assert m["num"].tolist() == [int((which == v).sum()) for v in range(3)]


# ---- 3. colliding keys ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("per_key", [1, 2])
def test_collision_fixture(host, dev, per_key):
    xyz, cov, _ = ref.collision_fixture(per_key)
    assert len(xyz) == 48 * per_key
    m = check_map(host, dev, xyz, cov)
    assert len(m["keys"]) == 48 and len({ref.hash_key(k) & 4095 for k in m["keys"].tolist()}) == 1
    src = (xyz.astype(np.float64) + 0.01).astype(F)
    sc, tc = ref.plain_cov(len(src)), ref.plain_cov(len(xyz))
    host.set_target(xyz, tc); dev.set_target(xyz, tc)                        # (covariances that invert well: the linearisation is compared next)
    host.set_source(src, sc); dev.set_source(src, sc)
    check_linearize(host, dev)
    _, _, _, nc = dev.linearize(np.eye(4), vgicp.DIRECT1)
    assert nc == len(src)                                                    # every key resolves, at the end of a 48-key probe chain too


# ---- 4. extreme voxel populations -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["one_voxel", "all_own", "counts_1_to_60"])
def test_extreme_populations(host, dev, kind):
    xyz, cov = ref.population_fixture(kind)
    m = check_map(host, dev, xyz, cov)
    if kind == "one_voxel":
        assert m["num"].tolist() == [2049]
    if kind == "all_own":
        assert len(m["num"]) == 3000 and (m["num"] == 1).all()
    if kind == "counts_1_to_60":
        assert sorted(m["num"].tolist()) == list(range(1, 61))


# ---- 5. synthetic scan pairs ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("given", [True, False])
@pytest.mark.parametrize("n", [2400, 14400])
def test_scan_pairs(host, dev, pairs, n, given):
    tx, tc, sx, sc, T_true = pairs[n]
    assert len(tx) == n
    if given:
        check_map(host, dev, tx, tc)
    else:                                                                    # the library's own covariance estimate: on the device it never comes down
        host.set_target(tx, None); dev.set_target(tx, None)
        mh, md = host.read_voxels(), dev.read_voxels()
        want = ref.build(tx, host.covariances(tx))
        for f in ("keys", "num", "mean", "cov", "wsq"):
            assert same(md[f], mh[f]) and same(md[f], want[f]), f
    host.set_source(sx, sc if given else None); dev.set_source(sx, sc if given else None)
    check_linearize(host, dev, (np.eye(4), T_true))
    for mode in MODES:
        o = host.default_options(neighbor_mode=mode)
        Th, sh = host.align(np.eye(4), o); Td, sd = dev.align(np.eye(4), o)
        assert same(Th, Td) and struct_bytes(sh) == struct_bytes(sd), mode
        assert sh.iterations > 0 and sh.n_correspondences > 0


# ---- 6. promotion -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("builder", [vgicp.BUILD_HOST, vgicp.BUILD_DEVICE])
def test_promote_source(so, pairs, builder):
    tx, _, sx, _, _ = pairs[2400]
    a, b = vgicp.Vgicp(so), vgicp.Vgicp(so)
    try:
        a.set_voxel_builder(builder)                                         # promotion is on the device whatever the builder
        a.set_source(tx); a.promote_source(0.5)
        # the source is still resident and linearises against its own map: every point finds its own voxel
        err, _, _, nc = a.linearize(np.eye(4), vgicp.DIRECT1)
        assert nc == len(tx) and np.isfinite(err)
        b.set_target(tx, None, 0.5)                                          # the host builder on a second context
        for f, v in a.read_voxels().items():
            assert same(v, b.read_voxels()[f]), f
        b.set_source(tx)
        assert lin_bytes(a, np.eye(4), vgicp.DIRECT7) == lin_bytes(b, np.eye(4), vgicp.DIRECT7)
        a.set_source(sx); b.set_source(sx)
        Ta, sa = a.align(np.eye(4)); Tb, sb = b.align(np.eye(4))
        assert same(Ta, Tb) and struct_bytes(sa) == struct_bytes(sb)
        assert sa.converged == 1
    finally:
        a.close(); b.close()


# ---- 7. one context, many sizes ---------------------------------------------------------------------------------------------------
def test_reuse_on_one_context(so, pairs):
    tx_s, tc_s = pairs[2400][0], pairs[2400][1]
    tx_l, tc_l = pairs[14400][0], pairs[14400][1]
    rng = np.random.default_rng(2)
    one = (np.array([[5.1, -3.3, 0.7]], F), ref.random_cov(rng, 1))
    used = vgicp.Vgicp(so); used.set_voxel_builder(vgicp.BUILD_DEVICE)
    maps = []
    try:
        used.set_source(pairs[2400][2], pairs[2400][3])
        for xyz, cov in ((tx_s, tc_s), (tx_l, tc_l), one, (tx_s, tc_s)):
            fresh = vgicp.Vgicp(so); fresh.set_voxel_builder(vgicp.BUILD_DEVICE)
            try:
                used.set_target(xyz, cov); fresh.set_target(xyz, cov)
                mu, mf = used.read_voxels(), fresh.read_voxels()
                for f in mu:
                    assert same(mu[f], mf[f]), (len(xyz), f)
                fresh.set_source(pairs[2400][2], pairs[2400][3])
                for mode in MODES:                                           # the table too: what a stale slot would corrupt
                    assert lin_bytes(used, T_SMALL, mode) == lin_bytes(fresh, T_SMALL, mode), (len(xyz), mode)
                maps.append(mu)
            finally:
                fresh.close()
        assert len(maps[2]["keys"]) == 1
        for f in maps[0]:
            assert same(maps[0][f], maps[3][f]), f
    finally:
        used.close()


# ---- 8. loop verification ---------------------------------------------------------------------------------------------------------
def test_loop_verify_under_both_builders(so, host, dev):
    query = vgicp.make_pair(0, rings=16, az=150)[2]
    cands = [(vgicp.make_pair(s, rings=16, az=150)[0], np.eye(4)) for s in (0, 1, 2)]
    ctx = lv.LoopVerify(so, max_points=2400)
    try:
        opts = lv.default_options(so)
        bh, ph = ctx.verify(host, query, cands, opts)
        bd, pd = ctx.verify(dev, query, cands, opts)
        assert struct_bytes(bh) == struct_bytes(bd)
        assert len(ph) == len(pd) == 3
        for a, b in zip(ph, pd):
            assert struct_bytes(a) == struct_bytes(b)
        assert max(p.iterations for p in pd) > 0
    finally:
        ctx.close()


# ---- 9. non-finite points ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("where", ["first", "last"])
@pytest.mark.parametrize("bad", [np.nan, np.inf])
def test_non_finite_points_leave_the_previous_target(dev, pairs, where, bad):
    tx, tc, sx, sc, _ = pairs[2400]
    dev.set_target(tx, tc); dev.set_source(sx, sc)
    before = [lin_bytes(dev, T_SMALL, mode) for mode in MODES]
    voxels = dev.read_voxels()
    broken = tx.copy(); broken[0 if where == "first" else len(tx) - 1, 1] = bad
    for cov in (tc, None):
        with pytest.raises(vgicp.VgicpError) as e:
            dev.set_target(broken, cov)
        assert e.value.status == vgicp.ERR_NON_FINITE
        assert [lin_bytes(dev, T_SMALL, mode) for mode in MODES] == before
    dev.set_source(broken, tc)
    with pytest.raises(vgicp.VgicpError) as e:
        dev.promote_source(0.5)
    assert e.value.status == vgicp.ERR_NON_FINITE
    dev.set_source(sx, sc)
    assert [lin_bytes(dev, T_SMALL, mode) for mode in MODES] == before
    for f, v in dev.read_voxels().items():
        assert same(v, voxels[f]), f


# ---- 10. argument errors ----------------------------------------------------------------------------------------------------------
def test_argument_errors(so, pairs):
    g = vgicp.Vgicp(so)
    try:
        for builder in (-1, 2, 7):
            with pytest.raises(vgicp.VgicpError) as e:
                g.set_voxel_builder(builder)
            assert e.value.status == vgicp.ERR_INVALID_ARGUMENT
        with pytest.raises(vgicp.VgicpError) as e:
            g.promote_source(0.5)                                            # no source yet
        assert e.value.status == vgicp.ERR_INVALID_ARGUMENT
        assert len(g.read_voxels()["keys"]) == 0 and g.voxel_count == 0      # no target yet: an empty map
        g.set_voxel_builder(vgicp.BUILD_DEVICE)
        g.set_target(pairs[2400][0], pairs[2400][1])
        n = len(g.read_voxels()["keys"])
        assert n > 1
        g.voxel_count = -1
        with pytest.raises(vgicp.VgicpError) as e:
            g.read_voxels(capacity=n - 1)
        assert e.value.status == vgicp.ERR_INVALID_ARGUMENT and g.voxel_count == n
        g.set_source(pairs[2400][2], pairs[2400][3])
        for res in (0.0, -1.0, float("nan")):
            with pytest.raises(vgicp.VgicpError) as e:
                g.promote_source(res)
            assert e.value.status == vgicp.ERR_INVALID_ARGUMENT
    finally:
        g.close()


def test_build_profile_counts_the_launches(dev, pairs):
    dev.build_profile_enable(True); dev.build_profile_read()
    dev.set_target(pairs[2400][0], pairs[2400][1]); dev.set_target(pairs[2400][0], pairs[2400][1])
    prof = dev.build_profile_read()
    dev.build_profile_enable(False)
    assert list(prof) == list(vgicp.BUILD_KERNELS)
    assert all(n == 2 and ms > 0.0 for n, ms in prof.values()), prof
    assert all(n == 0 and ms == 0.0 for n, ms in dev.build_profile_read().values())
