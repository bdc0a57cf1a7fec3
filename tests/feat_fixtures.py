"""The sequences the feature-tracker tests share and the NumPy reference on each, computed once (tests/feat_ref.py over the NumPy
restatements).  A case is (configuration, steps); a step is ("image", image, time_s, publish, seed) or ("reset",).  run() drives anything
with read_image / reset / snapshot through a case and returns one record per image."""
import functools

import numpy as np

import feat_ref as fr
from mvil_fusion_amd import track

F32 = np.float32


@functools.lru_cache(maxsize=None)
def scene(height, width, k):
    img = fr.scene_image(height, width, k)
    img.setflags(write=False)
    return img


def _steps(images, schedule=None, first_k=0):
    return [("image", img, fr.time_of(first_k + k), 1 if schedule is None else schedule[k], fr.seed_of(first_k + k)) for k, img in enumerate(images)]


def _scene_steps(cfg, n, schedule=None):
    return _steps([scene(cfg["height"], cfg["width"], k) for k in range(n)], schedule)


@functools.lru_cache(maxsize=None)
def case(name):
    S, L = fr.SMALL, fr.LARGE
    h, w = S["height"], S["width"]
    if name == "small_all":
        return S, _scene_steps(S, 6)
    if name == "small_schedule":
        return S, _scene_steps(S, 6, (1, 1, 0, 1, 0, 1))
    if name == "large_all":
        return L, _scene_steps(L, 4)
    if name == "large_skip2":
        return L, _scene_steps(L, 4, (1, 1, 0, 1))
    if name == "small_clahe":
        return dict(S, equalize=True), _scene_steps(S, 4)
    if name == "first_alone":
        return S, _scene_steps(S, 1)
    if name == "flat_then_texture":
        return S, _steps([np.full((h, w), 128, np.uint8), np.full((h, w), 128, np.uint8), scene(h, w, 0), scene(h, w, 1)])
    if name == "few_points":
        return dict(S, max_cnt=6), _scene_steps(S, 4)
    if name == "same_image_twice":
        return S, _steps([scene(h, w, 0), scene(h, w, 0), scene(h, w, 0), scene(h, w, 1)])
    if name == "unrelated_image":
        return S, _steps([scene(h, w, 0), scene(h, w, 1), track.Texture(h, w, seed=99).render(), scene(h, w, 3)])
    if name == "texture_then_flat":                             # on the image after the flat one every track is lost: n_before >= 8, n_tracked = 0
        return S, _steps([scene(h, w, 0), np.full((h, w), 128, np.uint8), scene(h, w, 2)])
    if name == "reset_mid":
        st = _scene_steps(S, 5)
        return S, st[:3] + [("reset",)] + st[3:]
    raise KeyError(name)


CASES = ("small_all", "small_schedule", "large_all", "large_skip2", "small_clahe", "first_alone", "flat_then_texture", "few_points", "same_image_twice", "unrelated_image",
         "texture_then_flat", "reset_mid")


def numpy_backend(cfg):
    return fr.NumpyBackend(cfg["width"], cfg["height"], fr.camera(cfg["width"], cfg["height"]), cfg["max_level"], max_iters=cfg["max_iters"], equalize=cfg.get("equalize", False))


def ref_tracker(cfg, backend):
    return RefAdapter(fr.FeatRef(backend, cfg["max_cnt"], cfg["min_dist"]))


class RefAdapter:
    """feat_ref.FeatRef behind the interface run() drives"""

    def __init__(self, ref):
        self.ref = ref

    def read_image(self, img, time_s, publish, seed):
        msg, s = self.ref.read_image(img, time_s, publish, seed)
        return msg, s, dict(self.ref.trace)

    def reset(self):
        self.ref.reset()

    def snapshot(self):
        r = self.ref
        return r.pts, r.ids, r.cnt, r.un, r.vel

    def level(self, which, l):
        return self.ref.b.level(which, l)


def run(tracker, steps, levels=None):
    """one record per image: msg, counts, pts, ids, cnt, un, vel, trace (None from a device) and, with levels = max_level, the pyramids"""
    out = []
    for st in steps:
        if st[0] == "reset":
            tracker.reset()
            continue
        _, img, t, pub, seed = st
        msg, counts, trace = tracker.read_image(img, t, pub, seed)
        pts, ids, cnt, un, vel = tracker.snapshot()
        rec = dict(msg={k: np.array(v) for k, v in msg.items()}, counts=dict(counts), pts=np.array(pts, F32), ids=np.array(ids, np.int32), cnt=np.array(cnt, np.int32),
                   un=np.array(un, F32), vel=np.array(vel, F32), trace=trace, publish=pub)
        if levels is not None:
            rec["levels"] = [np.array(tracker.level(which, l)) for which in ("cur", "forw") for l in range(levels + 1)]
        out.append(rec)
    return out


@functools.lru_cache(maxsize=None)
def reference(name):
    """the NumPy reference's records on a case, computed once and shared"""
    cfg, steps = case(name)
    return run(ref_tracker(cfg, numpy_backend(cfg)), steps, levels=cfg["max_level"] if cfg.get("equalize") else None)
