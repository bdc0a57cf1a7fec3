"""CPU checks of tests/clahe_ref.py, the NumPy restatement of include/vilclahe.h's contract: a known answer derived by hand, the
invariants of the redistribution and of the LUTs, and the conditions the fixtures of tests/clahe_fixtures.py must meet so that the
device's parity with the restatement (tests/test_gpu_clahe.py) cannot pass vacuously."""
import numpy as np

import clahe_fixtures as cf
import clahe_ref as cr


def test_permutation_tiles_have_the_answer_derived_by_hand():
    """Every 16 x 16 tile of a 128 x 128 image is a permutation of 0 .. 255, tiles 8 x 8, clip limit 3.0: area = 256, clip = 3 * 256 / 256 = 3,
    every bin holds 1 so nothing is clipped, the prefix sum at v is v + 1 and lut_scale = 255 / 256.  Every LUT is therefore
    rint((v + 1) * 255 / 256) half-even, and a blend of four equal values with weights that sum to 1 is that value: the output is that
    function of the input.  (v + 1) * 255 / 256 is exact in float32 (16 bits), so the expectation needs no float32 arithmetic at all: it is
    v + 1 - (v + 1) / 256 rounded to nearest, the tie at v + 1 = 128 (127.5) going to the even 128."""
    rng = np.random.default_rng(0)
    img = np.zeros((128, 128), np.uint8)
    for ty in range(8):
        for tx in range(8):
            img[16 * ty:16 * ty + 16, 16 * tx:16 * tx + 16] = rng.permutation(256).astype(np.uint8).reshape(16, 16)
    n = np.arange(1, 257)                                   # v + 1
    twice = 2 * n * 255                                     # 2 * 256 * the exact value: round to nearest, ties to even, in integers
    q, r = twice // 512, twice % 512
    lut = q + ((r > 256) | ((r == 256) & (q % 2 == 1)))
    assert lut[127] == 128 and lut[0] == 1 and lut[255] == 255 and lut[128] == 128 and lut[126] == 127       # 127.5 -> 128; 128.496 -> 128; 126.504 -> 127
    out, hists, L, stats, g = cr.apply(img, 8, 8, 3.0, full=True)
    assert g["clip"] == 3 and g["area"] == 256 and (g["we"], g["he"]) == (128, 128)
    assert all(s["clipped"] == 0 for row in stats for s in row)
    assert (L == lut.astype(np.uint8)[None, None, :]).all()
    # the blend's weights sum to 1 only up to rounding: with equal corner values V the result is within an ulp of V, and rint brings it back
    assert (out == lut.astype(np.uint8)[img]).all()


def test_geometry_pads_both_sides_when_either_is_not_divisible():
    g = cr.geometry(50, 64, 8, 8, 3.0)
    assert (g["he"], g["we"], g["th"], g["tw"], g["clip"]) == (56, 72, 7, 9, 1)
    g = cr.geometry(48, 67, 8, 8, 3.0)
    assert (g["he"], g["we"], g["th"], g["tw"]) == (56, 72, 7, 9)
    g = cr.geometry(61, 75, 8, 8, 3.0)
    assert (g["he"], g["we"], g["th"], g["tw"]) == (64, 80, 8, 10)
    g = cr.geometry(480, 640, 8, 8, 3.0)
    assert (g["he"], g["we"], g["th"], g["tw"], g["clip"]) == (480, 640, 60, 80, 56)
    assert cr.geometry(480, 640, 8, 8, 40.0)["clip"] == 750 and cr.geometry(480, 640, 8, 8, 0.0)["clip"] == 0
    assert cr.geometry(16, 16, 8, 8, 3.0)["clip"] == 1      # (int)(3 * 4 / 256) = 0, raised to 1
    img = np.arange(50 * 64, dtype=np.uint8).reshape(50, 64)
    ext = cr.extended(img, cr.geometry(50, 64, 8, 8, 3.0))
    assert ext.shape == (56, 72) and (ext[:50, :64] == img).all()
    assert (ext[50] == ext[48]).all() and (ext[55] == ext[43]).all() and (ext[:, 64] == ext[:, 62]).all() and (ext[:, 71] == ext[:, 55]).all()


def test_redistribution_conserves_the_sum_and_luts_are_monotone():
    for case in cf.CASES:
        out, hists, L, stats, g = cf.reference(*case)
        assert (hists.reshape(-1, 256).sum(axis=1) == g["area"]).all(), case
        assert (np.diff(L.astype(np.int64), axis=2) >= 0).all(), case
        assert (L[:, :, 255] == 255).all(), case            # the last prefix sum is area: rint(area * (255 / area)) = 255
        for row in stats:
            for s in row:
                assert s["clipped"] == 256 * s["batch"] + s["residual"] and 0 <= s["residual"] < 256
                assert s["step"] == (max(256 // s["residual"], 1) if s["residual"] else 0) and s["residual"] * s["step"] <= 256


def test_the_closed_form_is_the_loop():
    """bin i gets +1 iff i % step == 0 and i / step < residual, against the loop for (i = 0; i < 256 && residual > 0; i += step, residual--)"""
    for residual in range(1, 256):
        step = max(256 // residual, 1)
        loop = np.zeros(256, np.int64)
        i, r = 0, residual
        while i < 256 and r > 0:
            loop[i] += 1; i += step; r -= 1
        k = np.arange(256)
        assert (loop == ((k % step == 0) & (k // step < residual))).all() and loop.sum() == residual, residual


def test_clip_limit_zero_is_plain_per_tile_equalisation():
    h, w, tx, ty = 48, 64, 8, 8
    img = cf.image(h, w)
    out, hists, L, stats, g = cf.reference(h, w, tx, ty, 0.0)
    for j in range(ty):
        for i in range(tx):
            tile = img[6 * j:6 * j + 6, 8 * i:8 * i + 8]
            counts = np.bincount(tile.ravel(), minlength=256)
            assert (hists[j, i] == counts).all()
            cdf = np.cumsum(counts)                         # 255 * cdf / 48 = 85 * cdf / 16: round half-even in integers
            q, r = (85 * cdf) // 16, (85 * cdf) % 16
            want = q + ((r > 8) | ((r == 8) & (q % 2 == 1)))
            assert (L[j, i] == want).all()                  # lut_scale = 255 / 48 = 5.3125 and its products with cdf <= 48 are exact in float32


def test_a_strided_view_and_a_contiguous_copy_agree():
    img = cf.image(50, 64)
    wide = np.full((50, 96), 77, np.uint8); wide[:, :64] = img
    view = wide[:, :64]
    assert not view.flags["C_CONTIGUOUS"]
    assert (cr.apply(view) == cf.reference(50, 64, 8, 8, 3.0)[0]).all()
    rev = img[::-1, ::-1]                                   # negative strides
    assert (cr.apply(rev) == cr.apply(np.ascontiguousarray(rev))).all()


def test_fixtures_cover_the_branches_of_the_contract():
    flat = lambda case: [s for row in cf.reference(*case)[3] for s in row]
    everything = [s for case in cf.CASES for s in flat(case)]
    assert any(s["batch"] > 0 for s in everything)
    assert any(s["step"] == 1 for s in everything) and any(s["step"] == 2 for s in everything) and any(s["step"] >= 3 for s in everything)
    assert any(s["clipped"] == 0 for case in cf.CASES if case[4] > 0 for s in flat(case))            # an unclipped tile under a clip limit
    assert max(s["batch"] for s in flat((192, 256, 8, 8, 3.0))) == 2                                 # the flat tile: (768 - 9) / 256
    shapes = {c[:4] for c in cf.CASES}
    pads = {(h % ty != 0, w % tx != 0) for h, w, tx, ty in shapes}
    assert {(True, False), (False, True), (True, True), (False, False)} <= pads                      # rows only, columns only, both, none
    assert any(w % 4 for _, w, _, _ in shapes)              # a width the blend cannot take four bytes at a time
    # a tile of more than one workgroup's share (1024 pixels) and tiles below it
    areas = [cf.reference(*c)[4]["area"] for c in cf.CASES]
    assert max(areas) > 2048 and min(areas) == 4


def test_fixtures_tell_a_contracted_blend_from_the_contract():
    """A kernel compiled with FMA contraction evaluates step 4 as fused=True does; the fixtures hold enough pixels where that differs."""
    total = 0
    for case in cf.CASES:
        h, w, tx, ty, clip = case
        d = int((cr.apply(cf.image(h, w), tx, ty, clip, fused=True) != cf.reference(*case)[0]).sum())
        if case in ((192, 256, 8, 8, 3.0), (480, 640, 8, 8, 3.0), (48, 64, 8, 8, 3.0)):
            assert d >= 5, (case, d)
        total += d
    assert total >= 100
