"""The drives of tests/chain_cases.py, pinned with the oracle alone (no GPU).

The GPU test (tests/test_gpu_chain_fastpath.py) predicts from these cases how many corrections
the chain kernel's lean and generic programs run, message by message. For that to mean something
every case must contain exactly the rare events it claims, where it claims them, and nothing
else; the clean drives must contain none; and no angle may sit near normalize_angle_near's limit,
where the oracle's view (the heading before a correction) and the kernel's (after it) could differ.
"""
import numpy as np
import pytest

import chain_cases as cc
import edge_scenarios as es

_loc: dict = {}


def _locate(name, joseph=False):
    if (name, joseph) not in _loc:
        _loc[name, joseph] = cc.locate(cc.get(name), joseph)
    return _loc[name, joseph]


def test_shapes():
    """Maps of N = 20 and N = 130; messages of 1, 12, 16 and 20 markers (two chunks)."""
    assert {cc.get(n).n_landmarks for n in cc.CASES} == {20, 24, 130}
    want = {"clean_m1": 1, "clean_m12": 12, "clean_m16": 16, "clean_m20": 20, "clean_n130": 16}
    for name, m in want.items():
        assert np.all(cc.get(name).edge.count == m), name
    for name in cc.CASES:
        c = cc.get(name)
        assert c.start is not None and c.edge.n_messages == 4 and np.all(c.edge.actions == 0)


@pytest.mark.parametrize("joseph", [False, True], ids=["simple", "joseph"])
@pytest.mark.parametrize("name", cc.CLEAN)
def test_clean_drives_hold_no_event(name, joseph):
    o = _locate(name, joseph)
    assert o["events"] == {} and o["all_events"] == []
    assert np.all(o["rcs"] == 0) and o["margin"] > 1.0
    counts = cc.expected_counts(cc.get(name), o["events"])
    assert np.array_equal(counts[:, 0], cc.get(name).edge.count) and np.all(counts[:, 1] == 0)


@pytest.mark.parametrize("joseph", [False, True], ids=["simple", "joseph"])
@pytest.mark.parametrize("name", [n for n in cc.CASES if n not in cc.CLEAN])
def test_events_fall_where_claimed(name, joseph):
    """Each chunk's first event is the claimed one — position and kind — and chunks without a
    claim hold none; every event of the drive is a claimed mark (two_p3_p9: both of them)."""
    c, o = cc.get(name), _locate(name, joseph)
    assert c.claims and o["events"] == c.claims
    assert o["margin"] > 1.0
    kinds = {k for _, _, k in o["all_events"]}
    assert kinds == {k for _, k in c.claims.values()}
    if name == "two_p3_p9":
        assert o["all_events"] == [(0, 3, "first"), (0, 9, "first")]
    else:
        assert len(o["all_events"]) == 1
    # an id out of range is the oracle's -2 for that marker and changes nothing; everything else 0
    want = np.zeros(c.edge.n_messages, np.int32)
    for (t, _), (_, kind) in c.claims.items():
        if kind == "range":
            want[t] = -2
    assert np.array_equal(o["rcs"], want)
    counts = cc.expected_counts(c, o["events"])
    assert np.array_equal(counts.sum(1), c.edge.count)
    for (t, k), (p, _) in c.claims.items():
        m = min(cc.CHUNK, int(c.edge.count[t]) - k * cc.CHUNK)
        assert counts[t, 1] == m - p and counts[t, 1] >= 1
    assert counts[:, 1].sum() == sum(min(cc.CHUNK, int(c.edge.count[t]) - k * cc.CHUNK) - p
                                     for (t, k), (p, _) in c.claims.items())


def test_claimed_positions():
    """The first, a middle and the last position of a 16-marker chunk; the second chunk of a
    20-marker message; mid-chunk for the id out of range."""
    assert cc.get("first_p0").claims == {(0, 0): (0, "first")}
    assert cc.get("first_p7").claims == {(0, 0): (7, "first")}
    assert cc.get("first_p15").claims == {(0, 0): (15, "first")}
    assert cc.get("first_m20_p17").claims == {(0, 1): (1, "first")}
    assert cc.get("first_n130_p5").claims == {(0, 0): (5, "first")}
    assert cc.get("two_p3_p9").claims == {(0, 0): (3, "first")}
    assert cc.get("badid_p5").claims == {(1, 0): (5, "range")} and cc.get("badid_p5").how == "device"
    e = cc.get("badid_p5").edge
    assert e.ids[1, 5] >= e.n_landmarks


@pytest.mark.parametrize("name", cc.EDGE_CASES)
def test_edge_scenarios_events(name):
    """edge_scenarios' drives start from an empty map: the events are the first report of each id
    (message 0 is nothing else, so each of its chunks has one at position 0; the landmark a
    range-0 marker displaced from message 0 comes in message 1), the range-0 markers of the Z
    drives among them — first sightings whose S is then singular — and nothing else: H's headings
    are wrapped by the predict, S's seam lies well inside normalize_angle_near's range. The simple
    and the Joseph form see the same events."""
    c, o = cc.get(name), _locate(name)
    e = c.edge
    assert o["events"] == _locate(name, True)["events"]
    seen, firsts = set(), []
    for t in range(e.n_messages):
        for i in range(int(e.count[t])):
            if int(e.ids[t, i]) not in seen:
                seen.add(int(e.ids[t, i]))
                firsts.append((t, i, "first"))
    assert o["all_events"] == firsts
    assert set(e.zeros) <= {(t, i) for t, i, _ in firsts}
    for k in range((int(e.count[0]) + cc.CHUNK - 1) // cc.CHUNK):
        assert o["events"][0, k] == (0, "first")
    for t, p in e.zeros:
        assert o["events"][t, p // cc.CHUNK][0] <= p % cc.CHUNK
        if t > 0:
            assert o["events"][t, p // cc.CHUNK] == (p % cc.CHUNK, "first")
    assert np.array_equal(o["rcs"], es.expected_rcs(e))
    assert o["margin"] > 1.0
    run = es.run_oracle(e)   # the marker-by-marker pass is the message-level oracle's run
    assert np.array_equal(run["state"], o["state"]) and np.array_equal(run["sigma"], o["sigma"])


@pytest.mark.parametrize("turns", [5, -5])
def test_heading_state_events(turns):
    """ekf_set_state with a heading of about +-31 rad and no predict: the first correction's
    angles lie beyond normalize_angle_near's range (by more than a radian), every later one's
    well inside."""
    for joseph in (False, True):
        kinds, margin = cc.locate_heading_state(es.heading_state(turns), joseph)
        assert kinds[0] == "angle" and all(k is None for k in kinds[1:]) and len(kinds) == 12
        assert margin > 1.0
