"""tests/feat_ref.py -- the composition of include/vilfeat.h -- over the NumPy restatements, on the CPU: the test scene reaches every branch
of readImage's bookkeeping (asserted as conditions, so that a device test cannot hide behind a scene that exercised nothing), and the
bookkeeping's invariants hold on it."""
import numpy as np
import pytest

import feat_fixtures as ff
import feat_ref as fr

F32, F64 = np.float32, np.float64
BOTH = ("small_all", "small_schedule")


def test_the_scene_reaches_every_branch():
    recs = ff.reference("small_all")
    cfg = fr.SMALL
    later = recs[1:]
    assert recs[0]["counts"]["n_before"] == 0 and recs[0]["counts"]["n_new"] == cfg["max_cnt"] and recs[0]["counts"]["n_rows"] == 0      # a first image: detection only
    assert any(r["trace"]["lost"] > 0 for r in later), "no track is ever lost by LK"
    assert any(r["trace"]["rejected"] > 0 and r["counts"]["found"] for r in later), "the RANSAC never rejects a point"
    assert any(r["counts"]["found"] and 0 < r["counts"]["consumed"] < cfg["max_iters"] for r in later), "no adaptive stop before max_iters"
    assert any(r["counts"]["found"] and r["counts"]["consumed"] == cfg["max_iters"] for r in later), "the loop never runs to max_iters"
    assert any(r["trace"]["dropped"] > 0 for r in later), "setMask never drops a track"
    assert any(r["counts"]["n_new"] > 0 for r in later), "no refill"
    assert not recs[1]["vel"].any() and recs[1]["counts"]["n_rows"] > 0, "the second published image has a velocity that is not zero"
    assert any(r["vel"].any() for r in recs[2:]), "no velocity is ever non-zero"
    tie_matters = False
    for r in later:                                         # ties in track_cnt (an unstable sort may reorder them) next to counts that differ
        ids, cnt = r["trace"]["after_lk"]
        tie_matters |= len(set(cnt.tolist())) >= 3 and len(cnt) > len(set(cnt.tolist()))
    assert tie_matters, "no image has both ties in track_cnt and three different counts"
    sched = ff.reference("small_schedule")
    assert [r["publish"] for r in sched] == [1, 1, 0, 1, 0, 1]
    assert any(not r["publish"] and r["trace"]["lost"] > 0 and r["vel"].any() for r in sched), "no unpublished image loses a track and carries velocities"
    big = ff.reference("large_all")
    assert max(r["counts"]["n"] for r in big) > 256 and any(r["counts"]["found"] and r["counts"]["consumed"] < fr.LARGE["max_iters"] for r in big)


@pytest.mark.parametrize("name", BOTH)
def test_ids_are_unique_and_handed_out_in_index_order_without_gaps(name):
    next_id = 0
    for r in ff.reference(name):
        ids, pre = r["ids"], r["trace"]["ids_pre"]
        assert len(set(ids.tolist())) == len(ids)
        fresh = pre == -1
        assert (ids[fresh] == next_id + np.arange(int(fresh.sum()))).all()      # in index order, no gap
        assert (ids[~fresh] == pre[~fresh]).all()
        next_id += int(fresh.sum())
        assert r["counts"]["next_id"] == next_id
        if r["publish"]:
            assert (np.flatnonzero(fresh) >= r["counts"]["n_kept"]).all()         # addPoints appends


@pytest.mark.parametrize("name", BOTH)
def test_track_cnt_grows_by_one_per_image_published_or_not(name):
    prev = {}
    for r in ff.reference(name):
        now = dict(zip(r["ids"].tolist(), r["cnt"].tolist()))
        for i, c in now.items():
            assert c == prev[i] + 1 if i in prev else c == 1, (i, c, prev.get(i))
        prev = now


@pytest.mark.parametrize("name", BOTH)
def test_message_rows_are_the_points_seen_twice_in_state_order(name):
    for r in ff.reference(name):
        m, rows = r["msg"], (r["cnt"] > 1) if r["publish"] else np.zeros(len(r["cnt"]), bool)
        assert r["counts"]["n_rows"] == int(rows.sum()) == len(m["id"])
        assert m["id"].dtype == F32 and m["id"].tobytes() == r["ids"][rows].astype(F32).tobytes()
        assert m["points_xyz"].tobytes() == np.concatenate([r["un"][rows], np.ones((int(rows.sum()), 1), F32)], axis=1).astype(F32).tobytes()
        assert m["u"].tobytes() == r["pts"][rows, 0].tobytes() and m["v"].tobytes() == r["pts"][rows, 1].tobytes()
        assert m["vx"].tobytes() == r["vel"][rows, 0].tobytes() and m["vy"].tobytes() == r["vel"][rows, 1].tobytes()


@pytest.mark.parametrize("name", BOTH)
def test_velocities_are_zero_without_a_previous_entry_and_the_rounded_quotient_with_one(name):
    table, prev_t = {}, 0.0
    _, steps = ff.case(name)
    for r, st in zip(ff.reference(name), steps):
        pre, t = r["trace"]["ids_pre"], st[2]
        for i, pid in enumerate(pre.tolist()):
            if pid == -1 or pid not in table:
                assert not r["vel"][i].any(), (i, pid, r["vel"][i])
            else:
                want = ((r["un"][i].astype(F64) - table[pid].astype(F64)) / F64(t - prev_t)).astype(F32)
                assert r["vel"][i].tobytes() == want.tobytes()
        table = {}
        for i, pid in enumerate(pre.tolist()):               # keyed by the ids BEFORE updateID; the first occurrence stays
            table.setdefault(pid, r["un"][i])
        prev_t = t


@pytest.mark.parametrize("name", BOTH)
def test_priority_order_is_stable_count_descending_and_n_stays_within_max_cnt(name):
    for r in ff.reference(name):
        assert r["counts"]["n"] <= fr.SMALL["max_cnt"]
        if not r["publish"]:
            assert r["trace"]["priority"] is None
            continue
        p = r["trace"]["priority"]
        assert (np.diff(p) <= 0).all()
        ids, cnt = r["trace"]["after_lk"]                    # before the RANSAC: the survivors keep their relative order among equal counts
        pos = {i: k for k, i in enumerate(ids.tolist())}
        kept_ids = r["ids"][:r["counts"]["n_kept"]].tolist()
        kept_cnt = r["cnt"][:r["counts"]["n_kept"]].tolist()
        for a in range(len(kept_ids) - 1):
            if kept_cnt[a] == kept_cnt[a + 1]:
                assert pos[kept_ids[a]] < pos[kept_ids[a + 1]]


def test_an_unpublished_image_changes_neither_ids_nor_order_beyond_lks_compaction():
    recs = ff.reference("small_schedule")
    for prev, r in zip(recs[:-1], recs[1:]):
        if r["publish"]:
            continue
        ids, cnt = r["trace"]["after_lk"]
        assert (r["ids"] == ids).all() and (r["cnt"] == cnt).all() and r["counts"]["next_id"] == prev["counts"]["next_id"]
        it = iter(prev["ids"].tolist())                     # a subsequence of the previous ids, in order
        assert all(i in it for i in r["ids"].tolist())
        c = r["counts"]
        assert (c["found"], c["best_hypothesis"], c["consumed"], c["n_kept"], c["n_candidates"], c["n_new"], c["n_rows"]) == (0, -1, 0, 0, 0, 0, 0)
        assert c["n_inliers"] == c["n_tracked"] == c["n"]
