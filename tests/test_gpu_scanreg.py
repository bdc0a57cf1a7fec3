"""GPU parity of the LOAM feature extraction (include/vilscan.h) with its float32 restatement (tests/scanreg_ref.py), through the C-ABI.
Steps 1-5 are compared bit for bit; the voxel-filtered cloud to 1 float32 ulp (one rounding of an fp64 mean: not a measured tolerance)."""
import os

import numpy as np
import pytest

import scanreg_ref as ref
from mvil_fusion_amd import abi, lib, mapreg, scanreg, synth
from mvil_fusion_amd.vgicp import _rot

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
POSE = (_rot(-0.01, 0.015, -0.7), np.array([-2.0, 1.5, 0.2]))
SENSORS = {16: (-15.0, 15.0), 64: (-24.9, 2.0)}                     # scanRegistration.cpp:17, :686-689


def raw_bytes(a):
    return np.ascontiguousarray(a).view(np.uint8)


def ulp_diff(a, b):
    """Distance in float32 representable numbers (finite inputs)."""
    def key(x):
        i = np.ascontiguousarray(x, np.float32).view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7fffffff), i)
    return np.abs(key(a) - key(b))


def check(g, o, what=""):
    """g: scanreg.Features from the GPU, o: the restatement's result."""
    assert np.array_equal(g.ring_table, o.ring_table), what
    for name in ("cloud", "labels", "corner_sharp", "corner_less_sharp", "surf_flat"):
        a, b = getattr(g, name), getattr(o, name)
        assert a.shape == b.shape and np.array_equal(raw_bytes(a), raw_bytes(b)), (what, name, a.shape, b.shape)
    assert g.n_less_flat_raw == o.n_less_flat_raw, what
    assert g.surf_less_flat.shape == o.surf_less_flat.shape, (what, g.surf_less_flat.shape, o.surf_less_flat.shape)
    if len(o.surf_less_flat):
        d = ulp_diff(g.surf_less_flat, o.surf_less_flat).max()
        print("%s: less-flat cells %d, max ulp distance %d" % (what, len(o.surf_less_flat), d))
        assert d <= 1, (what, d)


def ref_config(cfg):
    return ref.Config(num_rings=cfg.num_rings, lower=cfg.lower_bound_deg, upper=cfg.upper_bound_deg, S=cfg.num_scan_subregions, C=cfg.num_curvature_regions,
                      th=cfg.surf_curv_th, max_sharp=cfg.max_corner_sharp, max_less=cfg.max_corner_less_sharp, max_flat=cfg.max_surf_flat, leaf=cfg.less_flat_filter_size)


@pytest.fixture(scope="module")
def so():
    return lib.load_vilsolve()


@pytest.fixture(scope="module")
def regs(so):
    out = {}
    for rings, (lo, hi) in SENSORS.items():
        out[rings] = scanreg.ScanReg(so, scanreg.default_config(so, num_rings=rings, lower_bound_deg=lo, upper_bound_deg=hi))
    yield out
    for r in out.values():
        r.close()


@pytest.mark.parametrize("seed", [0, 1, 2])
@pytest.mark.parametrize("rings,az", [(16, 900), (16, 1800), (64, 1800)])
def test_parity_on_the_synthetic_room(regs, rings, az, seed):
    lo, hi = SENSORS[rings]
    R, t = _rot(0.01 * seed, -0.02, 0.3 + 0.5 * seed), np.array([1.0 - seed, -2.0 + 1.5 * seed, 0.2])
    raw = scanreg.make_raw_scan(R, t, seed=seed, rings=rings, az=az, lower=lo, upper=hi)
    g = regs[rings].extract(raw)
    o = ref.extract(raw, ref_config(regs[rings].cfg))
    assert len(o.corner_less_sharp) > 10 and len(o.surf_flat) > 100 and len(o.surf_less_flat) > 1000
    check(g, o, "%dx%d seed %d" % (rings, az, seed))


def beam(az_deg, rng_m, inten, ele=1.0):
    a, e = np.deg2rad(np.asarray(az_deg, np.float64)), np.deg2rad(ele)
    r = np.broadcast_to(np.asarray(rng_m, np.float64), a.shape)
    return np.stack([r * np.cos(e) * np.cos(a), r * np.cos(e) * np.sin(a), r * np.sin(e), np.broadcast_to(np.asarray(inten, np.float64), a.shape)], axis=1).astype(np.float32)


def edge_cases():
    rng = np.random.default_rng(11)
    R, t = POSE
    room = scanreg.make_raw_scan(R, t, seed=4, rings=16, az=300)
    cases = {"empty": np.zeros((0, 4), np.float32)}
    nf = room[:50].copy(); nf[::3, 0] = np.nan; nf[1::3, 1] = np.inf; nf[2::3, 2] = -np.inf
    cases["all_non_finite"] = nf
    out = room[:200].copy(); out[:, 2] = np.abs(out[:, 2]) + 4.0 * np.hypot(out[:, 0], out[:, 1])             # elevation > 75 degrees
    cases["all_outside_elevation"] = out
    cases["one_ring"] = room[5::16].copy()
    wall = lambda n: beam(np.linspace(60, 60 + 0.15 * (n - 1), n), 5.0 / np.sin(np.deg2rad(np.linspace(60, 60 + 0.15 * (n - 1), n))), 10.0 + rng.uniform(0, 3, n))
    cases["ring_of_2C+1"] = wall(11)
    cases["ring_of_2C+2"] = wall(12)
    cases["ring_of_2C+3_subregions_with_ep<=sp"] = wall(13)
    cases["short_ring_some_subregions_empty"] = wall(24)                                                    # 14 interior points over 8 subregions: sizes 1 and 2
    dup = room[3::16].copy(); dup = np.repeat(dup, 2, axis=0)                                                # every point twice: zero gaps, tied curvatures
    cases["duplicates"] = dup
    flat = beam(np.linspace(0, 90, 301), 6.0, 10.0); flat[:, :3] = flat[100, :3]                             # 301 copies of one point: every curvature 0
    cases["all_curvatures_tied"] = flat
    rng_m = np.full(40, 3.0); rng_m[35:] = 8.0
    cases["clamped_mask_write"] = beam(np.linspace(0, 11.7, 40), rng_m, 10.0)
    mix = room.copy(); mix[::7, 0] = np.nan; mix[5::11, 2] += 30.0
    cases["mixed_drops"] = mix
    return cases


@pytest.mark.parametrize("name", sorted(edge_cases()))
def test_edge_cases(regs, name):
    raw = edge_cases()[name]
    g = regs[16].extract(raw)
    o = ref.extract(raw, ref_config(regs[16].cfg))
    if name in ("empty", "all_non_finite", "all_outside_elevation"):
        assert len(o.cloud) == 0 and not o.ring_table.any()
    if name == "one_ring":
        assert (o.ring_table[:, 1] > 0).sum() == 1 and o.n_less_flat_raw > 0
    if name == "ring_of_2C+1":
        assert o.ring_table[8].tolist() == [0, 11] and o.n_less_flat_raw == 0
    if name == "short_ring_some_subregions_empty":
        assert 0 < o.n_less_flat_raw < 14
    if name == "duplicates":
        assert len(o.corner_less_sharp) > 0
    if name == "clamped_mask_write":
        assert np.all(o.masks[8][35:] == 1)
    check(g, o, name)


def test_capacity_one_short_is_invalid(regs):
    R, t = POSE
    raw = scanreg.make_raw_scan(R, t, seed=7, rings=16, az=900)                  # the golden fixture's scan: every cloud is non-empty
    g = regs[16].extract(raw)
    exact = dict(cloud=len(g.cloud), corner_sharp=len(g.corner_sharp), corner_less_sharp=len(g.corner_less_sharp), surf_flat=len(g.surf_flat),
                 surf_less_flat=len(g.surf_less_flat), labels=len(g.cloud), rings=16)
    check(regs[16].extract(raw, exact), ref.extract(raw), "exact capacities")
    for k, v in exact.items():
        assert v > 0
        with pytest.raises(scanreg.ScanRegError) as e:
            regs[16].extract(raw, dict(exact, **{k: v - 1}))
        assert e.value.status == -1, k
    with pytest.raises(scanreg.ScanRegError) as e:
        small = scanreg.ScanReg(regs[16].lib, max_points=len(raw) - 1)
        try:
            small.extract(raw)
        finally:
            small.close()
    assert e.value.status == -1


def test_over_long_ring_and_uneven_are_unsupported(so, regs):
    n = scanreg.MAX_RING_POINTS + 1
    az = np.linspace(0, 350, n)
    raw = beam(az, 5.0, 10.0)
    with pytest.raises(scanreg.ScanRegError) as e:
        regs[16].extract(raw)
    assert e.value.status == -6
    check(regs[16].extract(raw[:-1]), ref.extract(raw[:-1]), "ring at the cap")              # 4096 points on one ring: supported
    with pytest.raises(scanreg.ScanRegError) as e:
        scanreg.ScanReg(so, scanreg.default_config(so, uneven=1))
    assert e.value.status == -6


def snapshot(f):
    return b"".join(raw_bytes(getattr(f, k)).tobytes() for k in scanreg.CLOUDS + ("ring_table", "labels")) + bytes([f.n_less_flat_raw & 0xff])


def test_determinism(hip, so, regs):
    """Same scan, byte-identical results: twice in one context, in a second context, and interleaved with a vmap_align and a vil_solve
    on the same device."""
    R, t = POSE
    raw = scanreg.make_raw_scan(R, t, seed=6, rings=16, az=1800)
    other = scanreg.make_raw_scan(R, t, seed=7, rings=16, az=900)
    a = snapshot(regs[16].extract(raw))
    regs[16].extract(other)
    assert snapshot(regs[16].extract(raw)) == a
    second = scanreg.ScanReg(so)
    assert snapshot(second.extract(raw)) == a
    cm, sm = mapreg.make_map(seed=4, n_surf=12000, n_corner=2000)
    sc, ss = mapreg.make_scan(cm, sm, R, t, seed=5, n_surf=2500, n_corner=400)
    m = mapreg.MapReg(so, "vmap_"); m.set_map(cm, sm)
    w = synth.make_config(1)
    for _ in range(5):
        m.align(hip.ctx, sc, ss, mapreg.quat_from_R(R), t + 0.03)
        assert snapshot(regs[16].extract(raw)) == a
        hip.solve(w, abi.default_options(max_iterations=4))
        assert snapshot(second.extract(raw)) == a
    m.close(); second.close()


def test_non_default_config(so):
    cfg = scanreg.default_config(so, num_scan_subregions=6, num_curvature_regions=3, max_corner_sharp=2, max_corner_less_sharp=20, max_surf_flat=6)
    reg = scanreg.ScanReg(so, cfg)
    R, t = POSE
    for seed in (0, 1):
        raw = scanreg.make_raw_scan(R, t, seed=seed, rings=16, az=1800)
        check(reg.extract(raw), ref.extract(raw, ref_config(cfg)), "S=6 C=3 quotas 2/20/6 seed %d" % seed)
    reg.close()


def test_gpu_reproduces_golden_fixture(regs):
    gold = np.load(os.path.join(HERE, "golden", "scanreg", "scan16x900.npz"))
    g = regs[16].extract(gold["raw"])
    assert np.array_equal(g.labels, gold["labels"]) and np.array_equal(g.ring_table, gold["ring_table"])
    assert g.n_less_flat_raw == int(gold["n_less_flat_raw"]) and len(g.surf_less_flat) == int(gold["n_less_flat"])


def test_profile_counts_every_kernel(regs):
    R, t = POSE
    raw = scanreg.make_raw_scan(R, t, seed=8, rings=16, az=300)
    regs[16].profile_enable(True)
    regs[16].profile_read()
    for _ in range(3):
        regs[16].extract(raw)
    prof = regs[16].profile_read()
    regs[16].profile_enable(False)
    assert sorted(prof) == sorted(scanreg.KERNELS) and all(n == 3 and ms > 0 for n, ms in prof.values()), prof


# ---- end to end: raw scan -> vscan_extract -> vmap_align ------------------------------------------------------------------------
E2E_GUESS_DT, E2E_GUESS_ROT = np.array([0.06, -0.06, 0.052915]), np.deg2rad(1.0)      # |dt| = 0.10 m, 1 degree about z


def e2e_scene():
    cm, sm = mapreg.make_map(seed=4, n_surf=60000, n_corner=6000)
    R, t = POSE
    raw = scanreg.make_raw_scan(R, t, seed=9, rings=16, az=1800)
    q0 = mapreg.quat_from_R(R @ _rot(0.0, 0.0, E2E_GUESS_ROT)); t0 = t + E2E_GUESS_DT
    return cm, sm, R, t, raw, q0, t0


def pose_errors(q, tt, R, t):
    Rq = synth.quat_to_R(np.asarray(q) / np.linalg.norm(q))
    ang = np.arccos(np.clip((np.trace(R.T @ Rq) - 1.0) / 2.0, -1.0, 1.0))
    return float(np.linalg.norm(np.asarray(tt) - t)), float(ang)


def test_end_to_end_registration_from_a_raw_scan(hip, so, oracle, regs):
    """The features of a raw scan taken at a known pose register it against the room's map from a guess 0.10 m and 1 degree off: the
    result is closer to the truth than the guess in translation and in rotation (the chain restatement -> oracle's orc_vmap_align
    satisfies the same on the CPU, checked first), and the GPU features give the pose the restatement's features give (inputs equal up
    to the 1-ulp voxel means; tolerance: the one test_gpu_map.py uses between its two solve paths)."""
    cm, sm, R, t, raw, q0, t0 = e2e_scene()
    e_t0, e_r0 = pose_errors(q0, t0, R, t)
    assert abs(e_t0 - 0.10) < 1e-3 and abs(e_r0 - np.deg2rad(1.0)) < 1e-6
    o = ref.extract(raw)
    orc = mapreg.MapReg(oracle.lib, "orc_vmap_"); orc.set_map(cm, sm)
    qo, to, s_o = orc.align(None, o.corner_less_sharp, o.surf_less_flat, q0, t0)
    orc.close()
    e_to, e_ro = pose_errors(qo, to, R, t)
    print("guess %.4f m %.4f rad; oracle chain %.4f m %.4f rad (%d edges, %d planes)" % (e_t0, e_r0, e_to, e_ro, s_o.n_edge, s_o.n_plane))
    assert e_to < e_t0 and e_ro < e_r0
    g = regs[16].extract(raw)
    m = mapreg.MapReg(so, "vmap_"); m.set_map(cm, sm)
    qg, tg, s_g = m.align(hip.ctx, g.corner_less_sharp, g.surf_less_flat, q0, t0)
    qr, tr, s_r = m.align(hip.ctx, o.corner_less_sharp, o.surf_less_flat, q0, t0)
    m.close()
    e_tg, e_rg = pose_errors(qg, tg, R, t)
    print("gpu chain %.4f m %.4f rad (%d edges, %d planes); |dt| vs restatement features %.3e" % (e_tg, e_rg, s_g.n_edge, s_g.n_plane, np.abs(tg - tr).max()))
    assert e_tg < e_t0 and e_rg < e_r0
    assert (s_g.n_edge, s_g.n_plane, s_g.iterations) == (s_r.n_edge, s_r.n_plane, s_r.iterations)
    assert np.abs(tg - tr).max() < 1e-9 and np.abs(qg - qr).max() < 1e-9
