"""The simulator cases of tests/sim_cases.py, pinned on pyekf.synth's output alone (no GPU).

tests/test_gpu_sim_edges.py compares the device simulator with these host restatements: ids and
counts exactly. For that to mean something each case must reach the path it is named for (a count
below the marker limit, a tie inside the cut, a message with no marker, a SURVEY message after a
NEAREST one, ...) and must be decidable: no two competing distances, and no distance and the range,
closer than GAP = 1e-6 (sim_cases.guard). A case that fails a pin here is re-seeded, never compared
more loosely.
"""
import numpy as np
import pytest

import sim_cases as sc
from pyekf import synth


def _ids(case, t, f):
    return case.sw.ids[t, f, :case.sw.count[t, f]].tolist()


@pytest.mark.parametrize("name", sc.NAMES)
def test_case_is_decidable_and_restated(name):
    """The guard; synth's ids against the landmark-by-landmark restatement of the selection; the
    arrays' padding; the Sim keywords."""
    c = sc.get(name)
    sw = c.sw
    worst = sc.guard(c)
    print(f"{name}: worst gap {worst:.3g}")
    assert worst > sc.GAP
    T, F, M = sw.ids.shape
    assert F <= 3 and M == c.stride == c.sim_kw["marker_stride"]
    assert T <= 12 or name == "growth"
    want = sc.select(c, "survey")
    for t in range(T):
        for f in range(F):
            assert _ids(c, t, f) == want[t][f], (t, f)
    pad = np.arange(M)[None, None, :] >= sw.count[..., None]
    assert (sw.ids[pad] == -1).all() and (sw.actions[pad] == 0).all() and (sw.rel[pad] == 0.0).all()
    assert (sw.ids[~pad] >= 0).all()
    # the runs tile the drive
    assert c.bounds[0][0] == 0 and c.bounds[-1][1] == T
    assert all(a[1] == b[0] for a, b in zip(c.bounds, c.bounds[1:]))
    assert (sw.seeds == np.uint64(c.sim_kw["seed"]) + np.uint64(c.sim_kw["f0"]) +
            np.arange(F, dtype=np.uint64)).all()
    assert sw.wheel.shape[1] == c.sim_kw["ticks_per_msg"] and sw.cmd.shape[0] == T * sw.wheel.shape[1]
    assert c.n_map <= c.n_slots


@pytest.mark.parametrize("L", sc.SIZES)
def test_size_cases_fill_min_16_L(L):
    c = sc.get(f"size-{L}")
    assert c.n_map == L and c.n_slots == (1024 if L == 1023 else max(L, 2))
    assert (c.sw.count == min(16, L)).all() and c.nearest_only and c.parallel
    if L in (65, 1023):  # the last slot of the 64 sensing lanes is partly empty
        assert L % 64 != 0 and L > 64


@pytest.mark.parametrize("tpm", sc.TICKS)
def test_ticks_cases(tpm):
    c = sc.get(f"ticks-{tpm}")
    assert c.sw.wheel.shape == (5, tpm, 2) and c.n_map == c.n_slots == 64
    assert (c.sw.count == 16).all()
    # the drive moves: the poses of consecutive messages differ
    assert (np.abs(np.diff(c.sw.truth, axis=0)).max(2) > 0).all()
    small = sc.get("ticks-64-small")
    assert small.sw.wheel.shape[1] == 64 and small.n_slots == 40


def test_markers_cases():
    for m in (1, 15):
        c = sc.get(f"markers-{m}")
        assert (c.sw.count == m).all() and c.stride == m and c.n_map == 64
    c = sc.get("markers-1-small")
    assert (c.sw.count == 1).all() and c.n_map == c.n_slots == 40


@pytest.mark.parametrize("name", ["ties-16", "ties-15", "ties-cross"])
def test_ties_come_lower_index_first_and_the_cut_splits_a_pair(name):
    c = sc.get(name)
    m = c.m
    d = sc.distances(c)[:, 0]
    lm = c.sw.landmarks[0]
    first = 48 if name == "ties-cross" else 7
    assert (lm[:64] == lm[64:128]).all() and (lm[128:] == lm[first:first + 2]).all()
    assert (c.sw.count == m).all()
    cross = 0
    for t in range(d.shape[0]):
        ids = _ids(c, t, 0)
        dd = d[t, ids]
        assert (np.diff(dd) >= 0).all()
        eq = np.flatnonzero(np.diff(dd) == 0.0)
        assert eq.size >= m // 2 - 1            # pairs (and triples) of bit-equal distances
        for i in eq:
            assert ids[i] < ids[i + 1], (t, ids)
        # same lane, next slot (l, l + 64) in every message; another lane (l, 128 + j) in some
        assert any(ids[i + 1] == ids[i] + 64 for i in eq)
        cross += any(ids[i + 1] >= 128 for i in eq)
        # the landmarks left out at the cut's distance: all of a higher index than the one kept
        out = [l for l in range(130) if l not in ids and d[t, l] == dd[-1]]
        if m == 15:
            assert out and min(out) > max(l for l in ids if d[t, l] == dd[-1]), (t, ids, out)
    # (points 7 and 8 are never in range of this drive: only ties-cross ties across lanes)
    assert cross >= 3 if name == "ties-cross" else cross == 0
    if m == 15:  # the same drive: the first 15 of the 16
        full = sc.get("ties-16")
        assert (full.sw.ids[:, :, :15] == c.sw.ids).all()


def test_empty_cases():
    c = sc.get("empty")
    cnt = c.sw.count
    assert cnt[:, 0].tolist() == [1, 1, 1, 1, 0, 0, 0, 0, 0, 1, 1, 2]
    assert cnt[:, 1].tolist() == [2, 3, 3, 3, 4, 3, 4, 4, 4, 4, 4, 4]
    assert cnt[:, 2].tolist() == [1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 1, 1]
    assert ((cnt == 0).any(1) & (cnt > 0).any(1)).any()
    assert c.bounds == ((0, 5), (5, 12)) and cnt[4, 0] == 0 and cnt[5, 0] == 0
    assert c.n_map == 12 and c.n_slots == 40 and c.nearest_only and c.parallel
    c = sc.get("empty-tail")
    cnt = c.sw.count
    assert c.n_map == 20 and c.bounds == ((0, 12),)
    assert (cnt[-3:, 0] == 0).all() and cnt[-4, 0] > 0
    assert (cnt[-4:, 2] == 0).all() and cnt[-5, 2] > 0
    assert (cnt[:, 1] > 0).all()


def test_nearest_then_survey_tells_the_two_sighted_rules_apart():
    """The simulator's rule (only SURVEY messages sight) against "any message sights", which the
    host restatement had: they select different ids in messages 3, 4, 5 and 7."""
    c = sc.get("nearest-then-survey")
    assert c.sw.sense.tolist() == [0, 0, 0, 1, 1, 1, 0, 1] and c.m == 4 and not c.parallel
    d = sc.distances(c)
    assert ((d <= 2.0 * c.max_range).sum(2) > c.m).all()
    ours, other = sc.select(c, "survey"), sc.select(c, "any")
    assert [t for t in range(8) if ours[t] != other[t]] == [3, 4, 5, 7]
    for t in range(8):
        for f in range(2):
            assert _ids(c, t, f) == ours[t][f]
    # where nothing but SURVEY messages came before, the rules agree (the survey-first workloads)
    first = sc._make("survey-first", 40, 64, 2, 8, map_seed=5, seed=5, m=4, max_range=2.5,
                     sense=[1, 1, 1, 1, 0, 0, 0, 0])
    assert sc.select(first, "survey") == sc.select(first, "any")


def test_mixed_all():
    c = sc.get("mixed-all")
    sw = c.sw
    assert sw.sense.tolist() == [0, 1, 2, 1, 0, 1, 1, 2, 0, 1] and c.stride == 12 and c.m == 3
    assert (sw.count[sw.sense == sc.ALL] == 12).all() and (sw.count[sw.sense != sc.ALL] == 3).all()
    assert int((sw.actions == synth.DELETE).sum()) == 29
    assert (sw.actions[sw.sense != sc.ALL] == 0).all()
    s = np.flatnonzero(sw.sense == sc.SURVEY)
    assert s.max() > np.flatnonzero(sw.sense == sc.ALL).max() and s.min() > 0
    assert sc.select(c, "survey") != sc.select(c, "any")


def test_all_delete():
    c = sc.get("all-delete")
    sw = c.sw
    assert c.basic_world and c.n_map == 4 and (sw.count == 4).all()
    gone = (sw.actions == synth.DELETE).all(2)            # [T, F]
    assert gone.any() and (sw.actions == synth.ADD).any()
    # a run that begins with such messages, one that ends with one, and corrections after them
    for f in range(sw.n_filters):
        assert gone[c.bounds[0][0], f] and gone[c.bounds[0][1] - 1, f] and gone[c.bounds[1][0], f]
        assert not gone[-1, f]


def test_survey_fallback():
    c = sc.get("survey-fallback")
    sw = c.sw
    d = sc.distances(c)
    assert (sw.sense == sc.SURVEY).all() and (sw.count == 1).all()
    assert (d > 2.0 * c.max_range).all()
    assert (sw.ids[:, :, 0] == d.argmin(2)).all()
    assert all(np.unique(sw.ids[:, f, 0]).size > 1 for f in range(2))  # (it changes on the way)


@pytest.mark.parametrize("stride", [20, 65])
def test_stride_cases_draw_their_noise_at_the_stride(stride):
    c, base = sc.get(f"stride-{stride}"), sc.get("size-64")
    sw = c.sw
    assert c.stride == stride > 16 and not c.parallel and base.parallel
    assert (sw.ids[:, :, :16] == base.sw.ids).all() and (sw.count == base.sw.count).all()
    assert (sw.truth == base.sw.truth).all()
    # noise draw 2·(t·M + i) (+1 for y) of stream 2 on the exact body-frame position
    T, F, M = sw.ids.shape
    th, x, y = (sw.truth[:, :, k:k + 1] for k in range(3))
    lm = np.take_along_axis(np.broadcast_to(sw.landmarks, (T,) + sw.landmarks.shape),
                            np.maximum(sw.ids, 0)[..., None], 2)
    dx, dy = lm[..., 0] - x, lm[..., 1] - y
    bx, by = np.cos(th) * dx + np.sin(th) * dy, -np.sin(th) * dx + np.cos(th) * dy
    idx = (np.arange(T, dtype=np.uint64)[:, None, None] * np.uint64(M) +
           np.arange(M, dtype=np.uint64)[None, None, :]) * np.uint64(2)
    sg = c.sim_kw["sensor_sigma"]
    live = sw.ids >= 0
    nx = bx + sg * synth.rng_normal(sw.seeds[None, :, None], 2, idx)
    ny = by + sg * synth.rng_normal(sw.seeds[None, :, None], 2, idx + np.uint64(1))
    assert (sw.rel[..., 0][live] == nx[live]).all() and (sw.rel[..., 1][live] == ny[live]).all()
    assert not (sw.rel[1:, :, :16] == base.sw.rel[1:]).all()   # (message 0 draws the same indices)
    assert (sw.rel[0, :, :16] == base.sw.rel[0]).all()


def test_marker_stride_keyword_defaults_and_floors():
    """None and any stride up to the default M leave synth's output as it was."""
    base = sc.get("size-64").sw
    for ms in (None, 1, 16):
        sw = sc._size(64, "x", marker_stride=ms).sw
        for k in ("ids", "actions", "rel", "count", "truth"):
            assert np.array_equal(getattr(sw, k), getattr(base, k)), (ms, k)


def test_f0_seed_no_noise_and_growth():
    c = sc.get("f0-seed")
    assert c.sim_kw["f0"] == 3 and c.sim_kw["seed"] == 2 ** 63 + 12345
    assert c.sw.seeds.tolist() == [2 ** 63 + 12345 + 3, 2 ** 63 + 12345 + 4]
    assert c.sw.seeds.dtype == np.uint64
    c = sc.get("no-noise")
    sw = c.sw
    assert c.sim_kw["slip"] == 0.0 and c.sim_kw["sensor_sigma"] == 0.0
    T, F, M = sw.ids.shape
    for t in range(T):
        for f in range(F):
            th, x, y = sw.truth[t, f]
            p = sw.landmarks[f, sw.ids[t, f]]
            dx, dy = p[:, 0] - x, p[:, 1] - y
            assert (sw.rel[t, f, :, 0] == np.cos(th) * dx + np.sin(th) * dy).all()
            assert (sw.rel[t, f, :, 1] == -np.sin(th) * dx + np.cos(th) * dy).all()
    assert np.abs(sw.truth[:, 0] - sw.truth[:, 1]).max() == 0.0   # no slip: one true path
    c = sc.get("growth")
    assert [b - a for a, b in c.bounds] == [1, 1, 3, 2, 7]
    assert (c.sw.ids[:6] == sc.get("size-64").sw.ids).all()
