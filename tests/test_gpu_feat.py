"""include/vilfeat.h on the GPU: vfeat_read_image against tests/feat_ref.py -- over the NumPy restatements, and over the device wrappers of the
three rows chained through the host (the separate calls it replaces) -- on raw bytes after every image: the message arrays, n_rows, the
state (cur_pts, ids, track_cnt), cur_un_pts, pts_velocity and the summary's counts.  No tolerance anywhere."""
import ctypes as C
import hashlib
import os
import subprocess
import sys

import numpy as np
import pytest

import feat_fixtures as ff
import feat_ref as fr
from mvil_fusion_amd import feat, lib, track

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
F32 = np.float32


@pytest.fixture(scope="module")
def so():
    return lib.load_vilsolve()


class DeviceAdapter:
    """feat.FeatureTracker behind the interface feat_fixtures.run() drives; keeps every summary"""

    def __init__(self, ft):
        self.ft, self.summaries = ft, []

    def read_image(self, img, time_s, publish, seed):
        msg, s = self.ft.read_image(img, time_s, publish, seed)
        self.summaries.append(s)
        return msg, {k: getattr(s, k) for k in fr.COUNTS}, None

    def reset(self):
        self.ft.reset()

    def snapshot(self):
        return self.ft.debug_state() + self.ft.debug_un_vel()

    def level(self, which, l):
        return self.ft.debug_level(which, l)


def device_tracker(so, cfg, **over):
    kw = dict(max_level=cfg["max_level"], max_candidates=1 << 14, max_iters=cfg["max_iters"], equalize=cfg.get("equalize", False), max_cnt=cfg["max_cnt"],
              min_dist=cfg["min_dist"])
    kw.update(over)
    return feat.FeatureTracker(so, cfg["width"], cfg["height"], fr.camera(cfg["width"], cfg["height"]), **kw)


def chain_tracker(so, cfg):
    b = fr.DeviceBackend(so, cfg["width"], cfg["height"], fr.camera(cfg["width"], cfg["height"]), cfg["max_level"], max(8, cfg["max_cnt"]), max_candidates=1 << 14,
                         max_iters=cfg["max_iters"], equalize=cfg.get("equalize", False))
    return ff.ref_tracker(cfg, b), b


def same_records(dev, ref, what):
    assert len(dev) == len(ref), what
    for k, (d, r) in enumerate(zip(dev, ref)):
        where = "%s, image %d" % (what, k)
        assert d["counts"] == r["counts"], (where, d["counts"], r["counts"])
        for key in fr.CHANNELS:
            a, b = d["msg"][key], r["msg"][key]
            assert a.dtype == b.dtype == F32 and a.shape == b.shape and a.tobytes() == b.tobytes(), (where, "message", key, a, b)
        for key in ("pts", "ids", "cnt", "un", "vel"):
            a, b = d[key], r[key]
            assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), (where, key, a, b)
        for l, (a, b) in enumerate(zip(d.get("levels", ()), r.get("levels", ()))):
            assert a.shape == b.shape and a.tobytes() == b.tobytes(), (where, "pyramid", l)


def check_budget(cfg, summaries, steps):
    """the waits and the bus of every call, from its summary"""
    images = [st for st in steps if st[0] == "image"]
    for s, st in zip(summaries, images):
        pub = st[3]
        assert s.host_waits <= (2 if pub and s.n_before > 0 else 1), (s.host_waits, pub, s.n_before)
        assert s.host_waits == (2 if pub and s.n_before >= 8 else 1)
        assert s.bytes_up <= cfg["width"] * cfg["height"] + 256 and s.bytes_up == cfg["width"] * cfg["height"]
        ransac = s.host_waits == 2                          # without the hypotheses the record count (4 bytes) is not written either
        assert s.bytes_down == feat.HEADER_BYTES - (0 if ransac else 4) + 8 * s.n_records + feat.ROW_BYTES * s.n_rows
        assert ransac or s.n_records == 0
        assert s.n_records <= max(0, s.n_tracked - 7)      # counts rise strictly from 8 to n_tracked at most
        assert s.bytes_down <= feat.ROW_BYTES * cfg["max_cnt"] + feat.HEADER_BYTES + 8 * max(0, cfg["max_cnt"] - 7)       # the message plus the header


@pytest.mark.parametrize("name", ff.CASES)
def test_read_image_equals_the_composition_and_the_chain_of_separate_calls(so, name):
    cfg, steps = ff.case(name)
    levels = cfg["max_level"] if cfg.get("equalize") else None
    ft = device_tracker(so, cfg)
    dev = DeviceAdapter(ft)
    got = ff.run(dev, steps, levels)
    same_records(got, ff.reference(name), name + " against the NumPy composition")
    chain, backend = chain_tracker(so, cfg)
    same_records(got, ff.run(chain, steps, levels), name + " against the chain of separate calls")
    check_budget(cfg, dev.summaries, steps)
    backend.close(); ft.close()


def test_the_edge_cases_are_the_edge_cases():
    """what the cases' names promise, asserted on the reference so that the comparison above means something"""
    ref = ff.reference
    assert [r["counts"]["n"] for r in ref("flat_then_texture")[:2]] == [0, 0] and ref("flat_then_texture")[2]["counts"]["n_new"] == fr.SMALL["max_cnt"]
    few = ref("few_points")
    assert all(r["counts"]["n"] <= 6 and r["counts"]["consumed"] == 0 and r["counts"]["best_hypothesis"] == -1 for r in few) and few[-1]["counts"]["n_rows"] > 0
    twice = ref("same_image_twice")
    assert twice[1]["trace"]["lost"] == 0 and twice[1]["counts"]["found"] and twice[1]["counts"]["consumed"] == 1          # zero flow: the first hypothesis fits every point
    assert any(r["counts"]["n_kept"] == fr.SMALL["max_cnt"] and r["counts"]["n_new"] == 0 for r in twice)
    assert ref("unrelated_image")[2]["trace"]["lost"] >= 10 and any(r["counts"]["n_tracked"] >= 8 and not r["counts"]["found"] for r in ref("unrelated_image"))
    flat = ref("texture_then_flat")[2]["counts"]            # cur is the flat image: every template fails LK's eigenvalue test
    assert flat["n_before"] >= 8 and flat["n_tracked"] == 0 and flat["consumed"] == 0
    rm = ref("reset_mid")
    assert rm[3]["counts"]["n_before"] == 0 and rm[3]["ids"].min() == rm[2]["counts"]["next_id"] and not rm[3]["vel"].any()
    big = ref("large_skip2")
    assert big[2]["publish"] == 0 and big[2]["counts"]["n"] > 256


def test_too_many_candidates_is_unsupported_and_leaves_the_context_as_after_a_reset(so):
    cfg = fr.SMALL
    h, w = cfg["height"], cfg["width"]
    ft = device_tracker(so, cfg, max_candidates=240)
    dev = DeviceAdapter(ft)
    imgs = [ff.scene(h, w, k) for k in range(5)]
    got = ff.run(dev, [("image", imgs[k], fr.time_of(k), 1, fr.seed_of(k)) for k in (0, 1)])
    noisy = track.Texture(h, w, seed=9).render(noise=12.0, seed=2)
    into = ft.new_message()
    for a in into.values():
        a[...] = -7.0
    with pytest.raises(feat.FeatError) as e:
        ft.read_image(noisy, fr.time_of(2), True, fr.seed_of(2), into=into)
    assert e.value.status == -6
    assert all((a == -7.0).all() for a in into.values()), "an output was written"
    assert len(ft.debug_state()[1]) == 0
    got += ff.run(dev, [("image", imgs[k], fr.time_of(k), 1, fr.seed_of(k)) for k in (3, 4)])
    ref = ff.ref_tracker(cfg, ff.numpy_backend(cfg))
    steps = [("image", imgs[k], fr.time_of(k), 1, fr.seed_of(k)) for k in (0, 1)] + [("reset",)] + [("image", imgs[k], fr.time_of(k), 1, fr.seed_of(k)) for k in (3, 4)]
    want = ff.run(ref, steps)
    assert want[2]["counts"]["n_before"] == 0 and want[2]["counts"]["next_id"] > want[1]["counts"]["next_id"]
    same_records(got, want, "after VIL_ERR_UNSUPPORTED")
    ft.close()


def test_an_invalid_call_in_mid_sequence_changes_nothing(so):
    cfg, steps = ff.case("small_all")
    ft = device_tracker(so, cfg)
    dev = DeviceAdapter(ft)
    f = so.vfeat_read_image; f.restype = C.c_int
    img = np.ascontiguousarray(steps[0][1])
    into = ft.new_message()
    for a in into.values():
        a[...] = -7.0
    msg = feat.VfeatMsg(*[into[k].ctypes.data_as(C.POINTER(C.c_float)) for k in feat.CHANNELS], -1, 0)
    holed = feat.VfeatMsg(*[into[k].ctypes.data_as(C.POINTER(C.c_float)) for k in feat.CHANNELS], -1, 0); holed.vx = None
    s = feat.VfeatSummary(); s.n = -5
    p, W = C.c_void_p(img.ctypes.data), C.c_int32(cfg["width"])
    bad = ((None, W, 0.3, 1, msg), (p, C.c_int32(cfg["width"] - 1), 0.3, 1, msg), (p, W, float("nan"), 1, msg), (p, W, 0.3, 1, None), (p, W, 0.3, 1, holed))
    got = []
    for k, st in enumerate(steps):
        got += ff.run(dev, [st])
        for g, stride, t, pub, m in bad:
            assert f(ft.ctx, g, stride, C.c_double(t), C.c_int32(pub), C.c_uint64(5), C.byref(m) if m is not None else None, C.byref(s)) == -1
        assert s.n == -5 and msg.n_rows == -1 and all((a == -7.0).all() for a in into.values())
    same_records(got, ff.reference("small_all"), "with invalid calls in between")
    ft.close()


def run_chain(so):
    """the digest of everything two sequences leave: what a second context and a fresh process must reproduce"""
    h = hashlib.sha256()
    for name in ("small_schedule", "large_all"):
        cfg, steps = ff.case(name)
        ft = device_tracker(so, cfg)
        for r in ff.run(DeviceAdapter(ft), steps):
            for key in fr.CHANNELS:
                h.update(r["msg"][key].tobytes())
            for key in ("pts", "ids", "cnt", "un", "vel"):
                h.update(r[key].tobytes())
            h.update(repr(sorted(r["counts"].items())).encode())
        ft.close()
    return h.hexdigest()


def test_bit_reproducible_across_contexts_and_processes(so):
    a = run_chain(so)
    assert run_chain(so) == a
    out = subprocess.run([sys.executable, os.path.join(HERE, "feat_child.py")], check=True, capture_output=True, text=True, timeout=300).stdout
    assert "digest " + a in out, out


def test_profile_names_the_new_kernels(so):
    cfg, steps = ff.case("small_all")
    ft = device_tracker(so, cfg)
    ft.profile_enable(True)
    ff.run(DeviceAdapter(ft), steps[:3])
    prof = ft.profile_read()
    assert tuple(prof) == feat.KERNELS
    assert prof["k_feat_compact_lk"][0] == 3 and prof["k_feat_finish"][0] == 3 and prof["k_feat_compact_rank"][0] == 3 and prof["k_feat_compact_add"][0] == 3
    assert prof["k_feat_records"][0] == 2                   # not on the first image: no points
    assert all(ms > 0 for n, ms in prof.values())
    ft.close()
