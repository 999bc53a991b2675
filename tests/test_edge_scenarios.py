"""The rare-path scenarios of tests/edge_scenarios.py, pinned with the oracle alone (no GPU).

The GPU tests replay these scenarios through the product and compare with the structured oracle.
For that comparison to mean something, each scenario must do what it was built for (a skip exactly
at the planned messages, a heading beyond the fast normalisation's range, a raw innovation beyond
pi, ...) and must be well conditioned: the oracle's literal dense arithmetic and its structured
restatement — two faithful fp64 evaluation orders — have to agree ten times tighter than the bound
the GPU test applies, in the simple and the Joseph form, take the same association decisions, and
keep every decision at least 0.05 from the gate. A scenario that fails a pin is re-seeded, never
given a wider bound.
"""
import math

import numpy as np
import pytest

import edge_scenarios as es
import orc

ALL = list(es.KNOWN) + list(es.ASSOC) + list(es.ASSOC_MULTI)
_runs: dict = {}


def _run(name, literal=False, joseph=False):
    key = (name, literal, joseph)
    if key not in _runs:
        _runs[key] = es.run_oracle(es.get(name), literal=literal, joseph=joseph)
    return _runs[key]


@pytest.mark.parametrize("joseph", [False, True], ids=["simple", "joseph"])
@pytest.mark.parametrize("name", ["clean"] + ALL)
def test_scenario_is_well_conditioned(name, joseph):
    e = es.get(name)
    a, b = _run(name, False, joseph), _run(name, True, joseph)
    want = es.expected_rcs(e)
    for o in (a, b):
        assert np.array_equal(o["rcs"], want), o["rcs"]
        assert np.all(np.isfinite(o["state"])) and np.all(np.isfinite(o["sigma"]))
        assert np.all(np.isfinite(o["poses"]))
    assert np.array_equal(a["assoc_j"], b["assoc_j"])
    assert np.array_equal(a["assoc_new"], b["assoc_new"])
    assert a["counter"] == b["counter"]
    for o in (a, b):
        d = o["dmin"][np.isfinite(o["dmin"])]
        assert d.size == 0 or np.abs(d - es.GATE).min() >= 0.05
    pt, st, sg = es.ASSOC_TOL if e.assoc else es.KNOWN_TOL
    assert np.abs(a["poses"] - b["poses"]).max() <= pt / 10
    assert np.abs(a["state"] - b["state"]).max() <= st / 10
    assert np.abs(a["sigma"] - b["sigma"]).max() <= sg / 10


@pytest.mark.parametrize("name", ALL)
def test_forms_take_the_same_decisions(name):
    """The Joseph form differs from the simple one in rounding only: same skips, same decisions."""
    a, j = _run(name), _run(name, joseph=True)
    assert np.array_equal(a["rcs"], j["rcs"])
    assert np.array_equal(a["assoc_j"], j["assoc_j"])
    assert np.array_equal(a["assoc_new"], j["assoc_new"])


@pytest.mark.parametrize("name", [n for n in es.KNOWN if n.startswith("Z")])
def test_zero_range_first_sightings(name):
    """Each range-0 marker is the first and only report of a spare id; the skipped correction
    leaves its landmark where the first sighting put it: on the robot (slam.cpp:213-216)."""
    e = es.get(name)
    assert e.skips == (0, 6) and len(e.zeros) == 2
    live = np.arange(e.ids.shape[1])[None, :] < e.count[:, None]
    x = _run(name)["state"]
    for t, p in e.zeros:
        lid = int(e.ids[t, p])
        assert np.all(e.rel[t, p] == 0.0) and p < e.count[t]
        assert np.count_nonzero(live & (e.ids == lid)) == 1
        assert np.any(x[3 + 2 * lid:5 + 2 * lid] != 0.0)
    # every other landmark slot that was never reported is still (0, 0)
    seen = np.unique(e.ids[live])
    for lid in np.setdiff1d(np.arange(e.n_landmarks), seen):
        assert np.all(x[3 + 2 * lid:5 + 2 * lid] == 0.0)


def test_zero_range_chunk_positions():
    """The 16-marker message has its zero on a chunk's last marker (EKF_MAX_CHUNK = 16); the
    20-marker messages span two chunks, the zero last in the first or first in the second."""
    assert es.get("Z16_p15").zeros == ((0, 15), (6, 15)) and es.get("Z16_p15").count.min() == 16
    assert es.get("Z20_p15").zeros == ((0, 15), (6, 15)) and es.get("Z20_p15").count.min() == 20
    assert es.get("Z20_p16").zeros == ((0, 16), (6, 16)) and es.get("Z20_p16").count.min() == 20


@pytest.mark.parametrize("name", ["H_p25", "H_p20", "H_m25", "Z12_p3_p20", "A20_3_p25",
                                  "A130_last_p25"])
def test_heading_leaves_the_fast_range(name):
    """The heading of t_map_odom * t_odom_robot (compose does not wrap) is beyond the |a + pi| <
    5 pi range in which normalize_angle needs no fmod, at least once, and the filter's own heading
    stays in (-pi, pi]."""
    o = _run(name)
    assert np.abs(o["raw_theta"] + math.pi).max() > 5 * math.pi
    assert np.all(np.abs(o["poses"][:, 0]) <= math.pi)


def test_seam_crossings():
    e = es.get("S_seam")
    raw, before, after = es.seam_trace(e)
    assert np.count_nonzero(np.abs(raw) > math.pi) >= 3
    flips = (np.sign(before) != np.sign(after)) & (np.abs(before) > 3.0) & (np.abs(after) > 3.0)
    assert np.count_nonzero(flips) >= 3
    # the heading the odometry reports is within 1e-4 of pi; landmark 3 is straight behind
    assert np.all(np.abs(e.odom[:, 0] - math.pi) < 1e-4)
    b = np.arctan2(e.rel[:, 1, 1], e.rel[:, 1, 0])
    assert np.allclose(np.abs(b), math.pi - 1e-3, atol=1e-12) and b[0] * b[1] < 0


@pytest.mark.parametrize("name", list(es.ASSOC))
def test_assoc_phantom_is_committed(name):
    """The range-0 marker sits in the last message only, opens a new landmark (counter + 1) and its
    correction is skipped; at position 3 a later marker of that message associates with it."""
    e = es.get(name)
    o = _run(name)
    T = e.n_messages - 1
    (t, p), = e.zeros
    assert t == T and e.skips == (T,)
    assert np.all(e.rel[t, p] == 0.0)
    assert o["assoc_new"][T, p] == 1
    slot = int(o["assoc_j"][T, p])
    before = int(o["counters"][T - 1])
    assert slot >= before and o["counter"] == before + int(o["assoc_new"][T].sum())
    c = int(e.count[T])
    if p == c - 1:
        assert slot == o["counter"] - 1
    else:
        assert np.any(o["assoc_j"][T, p + 1:c] == slot)
    # three workgroups of 64 slots at N = 130, one at N = 20
    assert e.n_landmarks in (20, 130)


def test_assoc_multi_skips():
    """Two skipped markers in two messages, two in one message, and a skip followed by a clean
    message: each zero opens a landmark of its own."""
    a = es.get("A20_two_msgs")
    T = a.n_messages
    assert a.skips == (T - 2, T - 1) and [t for t, _ in a.zeros] == [T - 1, T - 2]
    b = es.get("A20_two_same")
    assert b.skips == (T - 1,) and sorted(b.zeros) == [(T - 1, 3), (T - 1, int(b.count[T - 1]) - 1)]
    c = es.get("A20_zero_then_clean")
    assert c.skips == (T - 2,) and c.zeros == ((T - 2, int(c.count[T - 2]) - 1),)
    for name in es.ASSOC_MULTI:
        e, o = es.get(name), _run(name)
        for t, p in e.zeros:
            assert np.all(e.rel[t, p] == 0.0) and o["assoc_new"][t, p] == 1
    assert _run("A20_two_msgs")["counter"] == _run("A20_two_same")["counter"] == 12
    assert _run("A20_zero_then_clean")["counter"] == 11
    for name in ("A20_zero_then_clean", "A130_zero_then_clean"):
        e, o = es.get(name), _run(name)   # the clean last message corrects the phantom landmark
        (t, p), = e.zeros
        assert o["assoc_j"][t, p] in o["assoc_j"][t + 1]
    # ... at N = 20 in a message that commits nothing itself
    assert _run("A20_zero_then_clean")["assoc_new"][-1].sum() == 0


@pytest.mark.parametrize("joseph", [False, True], ids=["simple", "joseph"])
@pytest.mark.parametrize("turns", [5, -5])
def test_heading_state_without_predict(turns, joseph):
    """ekf_set_state + ekf_correct with no predict: the first correction sees a heading of about
    +-31 rad, every later one a wrapped heading; the oracle's two modes agree ten times tighter
    than the bound."""
    hs = es.heading_state(turns)
    # |atan2(..) - theta + pi| >= |theta| - 2 pi: the bearing and the heading are both beyond 5 pi
    assert abs(hs[0][0]) > 7 * math.pi
    xa, Sa, ta, th = es.run_heading_state(hs, False, joseph)
    xb, Sb, tb, _ = es.run_heading_state(hs, True, joseph)
    assert np.all(np.abs(th[:, 0]) <= math.pi)   # wrapped by the first correction already
    assert np.all(np.isfinite(Sa)) and np.all(np.isfinite(Sb))
    assert np.abs(xa - xb).max() <= es.KNOWN_TOL[1] / 10
    assert np.abs(ta - tb).max() <= es.KNOWN_TOL[1] / 10
    assert np.abs(Sa - Sb).max() <= es.KNOWN_TOL[2] / 10


@pytest.mark.parametrize("N", list(es.LAST_SLOT))
def test_last_slot_landmark_commits(N):
    """From the oracle's own known-id survey with slot N - 1 reset to the prior and counter N - 1:
    markers associate with mapped landmarks, the relabelled landmark is the one commit, on slot
    N - 1, and every decision stays 0.05 from the gate."""
    sc = es.last_slot_scenario(N)
    odom = es.oracle_odometry(sc)
    w = sc.n_warm
    ref = orc.OracleEKF(n_landmarks=N)
    for t in range(w):
        ref.set_odom(odom[t])
        c = int(sc.count[t])
        assert ref.fake_sensor_cb(sc.ids[t, :c], sc.actions[t, :c], sc.rel[t, :c]) == 0
    x, S, tmo, _ = ref.get()
    es.forget_last(x, S)
    ref.set(x, S, tmo, x[:3], N - 1)
    commits, n_old = [], 0
    for t in range(w, sc.n_messages):
        ref.set_odom(odom[t])
        rc, j, nw, dmin = ref.sensor_cb_dmin(sc.rel[t, :int(sc.count[t])])
        assert rc in (0, -2)
        d = dmin[np.isfinite(dmin)]
        assert d.size == 0 or np.abs(d - es.GATE).min() >= 0.05
        commits += [int(a) for a in j[nw == 1]]
        n_old += int(np.count_nonzero((j >= 0) & (nw == 0)))
    assert commits == [N - 1] and n_old > 0
