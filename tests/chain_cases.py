"""Drives for the two programs of k_chain's sequential wave, and where their rare events fall.

The chain kernel runs a chunk's corrections in a lean program that holds the common case alone and
hands the chunk to the generic program at the first marker that is anything else: a first sighting
(the landmark still at (0, 0), slam.cpp:213-216), an id out of range, a singular or non-finite S
(the oracle's -4), a bearing or heading beyond normalize_angle_near's range. The builders here give
small drives with such an event at a chosen position of a chosen chunk, or with none; `locate`
finds every event of a drive with the oracle alone (predict / correct / posterior, marker by
marker), so that tests/test_chain_cases.py can pin each case to what it claims, and the GPU test
(tests/test_gpu_chain_fastpath.py) can predict the kernel's step counters from it.

A case starts from a populated map: the oracle's state after the drive's first `pre` messages
(loaded with ekf_set_state), with some landmarks withheld (`forget`: back to the prior, so their
next sighting is a first one).
"""
from __future__ import annotations

import math
from dataclasses import dataclass, field

import numpy as np

import edge_scenarios as es
import orc
from pyekf import synth

CHUNK = 16          # EKF_MAX_CHUNK: markers of one chunk
FIVE_PI = 5.0 * math.pi


@dataclass
class Case:
    name: str
    edge: es.Edge                  # the messages under test (after the first `pre` of the drive)
    start: tuple | None            # (x, S, tmo, counter) to load first; None: a fresh filter
    claims: dict = field(default_factory=dict)   # {(message, chunk): (position, kind)} by design
    how: str = "sensor"            # "sensor": ekf_fake_sensor per message; "device":
                                   # ekf_replay_device (one upload; ids reach the kernel unchecked)

    @property
    def n_landmarks(self) -> int:
        return self.edge.n_landmarks


def forget(x, S, lid, prior=10e6):
    """Landmark `lid` back to the prior (slam.cpp:127-132), in place."""
    k = 3 + 2 * lid
    x[k:k + 2] = 0.0
    S[k:k + 2, :] = 0.0
    S[:, k:k + 2] = 0.0
    S[k, k] = S[k + 1, k + 1] = prior


def _tail(e: es.Edge, pre: int, name: str) -> es.Edge:
    return es.Edge(name, e.n_landmarks, e.count[pre:].copy(), e.ids[pre:].copy(),
                   e.actions[pre:].copy(), e.rel[pre:].copy(), e.odom[pre:].copy())


_full: dict = {}


def _drive(key):
    """→ (the whole drive as an Edge, the oracle's state after its first `pre` messages, pre).
    key: 12 / 16 / 20 markers per message in a 20 / 20 / 24-slot filter (edge_scenarios' base
    drive: every message reports the same ids), or "n130": 130 slots, every landmark surveyed."""
    if key not in _full:
        if key == "n130":
            sc = synth.populated(130, 5)
            pre = sc.n_warm
            e = es._edge("n130", sc)
        else:
            e = es._edge(f"base{key}", es._base(key))
            pre = 2
        assert np.all(e.actions == 0)
        ref = orc.OracleEKF(n_landmarks=e.n_landmarks)
        for t in range(pre):
            ref.set_odom(e.odom[t])
            c = int(e.count[t])
            assert ref.fake_sensor_cb(e.ids[t, :c], e.actions[t, :c], e.rel[t, :c]) == 0
        _full[key] = (e, ref.get(), pre)
    e, (x, S, tmo, cnt), pre = _full[key]
    return e, (x.copy(), S.copy(), tmo.copy(), cnt), pre


def populated(name, key, n_msgs=4, count=None, withheld=(), bad=()):
    """The drive `key` from its populated state, `n_msgs` messages. count: messages cut to that many
    markers. withheld: (message, position) pairs — the landmark reported there is forgotten in the
    start state, so that marker is its first sighting (message 0 for the base drives, whose every
    message reports every landmark). bad: (message, position, id) — an id out of range there."""
    e, (x, S, tmo, cnt), pre = _drive(key)
    t = _tail(e, pre, name)
    t = es.Edge(name, t.n_landmarks, t.count[:n_msgs], t.ids[:n_msgs], t.actions[:n_msgs],
                t.rel[:n_msgs], t.odom[:n_msgs])
    if count is not None:
        assert np.all(t.count >= count)
        t.count[:] = count
    claims = {}
    for m, p in withheld:
        forget(x, S, int(t.ids[m, p]))
    for m, p, lid in bad:
        t.ids[m, p] = lid
    marks = [(m, p, "first") for m, p in withheld] + [(m, p, "range") for m, p, _ in bad]
    for m, p, kind in sorted(marks):  # a chunk's earliest event is the one that counts
        claims.setdefault((m, p // CHUNK), (p % CHUNK, kind))
    return Case(name, t, (x, S, tmo, cnt), claims, "device" if bad else "sensor")


def from_edge(name) -> Case:
    """A scenario of edge_scenarios.py from a fresh filter (its first message is all first
    sightings; the Z scenarios add range-0 first sightings of spare ids)."""
    return Case(name, es.get(name), None)


CASES = {
    # no event at all: messages of 1, 12 and 16 markers, of 20 (two chunks), and the 130-slot map
    "clean_m1": lambda: populated("clean_m1", 12, count=1),
    "clean_m12": lambda: populated("clean_m12", 12),
    "clean_m16": lambda: populated("clean_m16", 16),
    "clean_m20": lambda: populated("clean_m20", 20),
    "clean_n130": lambda: populated("clean_n130", "n130"),
    # a landmark withheld from the map: first sighting at the first, a middle and the last position
    # of a 16-marker chunk; in the second chunk of a 20-marker message; on the 130-slot map
    "first_p0": lambda: populated("first_p0", 16, withheld=((0, 0),)),
    "first_p7": lambda: populated("first_p7", 16, withheld=((0, 7),)),
    "first_p15": lambda: populated("first_p15", 16, withheld=((0, 15),)),
    "first_m20_p17": lambda: populated("first_m20_p17", 20, withheld=((0, 17),)),
    "first_n130_p5": lambda: populated("first_n130_p5", "n130", withheld=((0, 5),)),
    # two rare events in one chunk
    "two_p3_p9": lambda: populated("two_p3_p9", 16, withheld=((0, 3), (0, 9))),
    # an id out of range in mid-chunk (only a device replay hands one to the kernel)
    "badid_p5": lambda: populated("badid_p5", 16, bad=((1, 5, 20 + 3),)),
}
CLEAN = [n for n in CASES if n.startswith("clean_")]
# edge_scenarios' drives the GPU test replays too (imported, not edited)
EDGE_CASES = ["Z12_p0", "Z12_p3", "Z12_p11", "Z16_p15", "Z20_p16", "H_p25", "S_seam"]
_cache: dict = {}


def get(name) -> Case:
    if name not in _cache:
        _cache[name] = CASES[name]() if name in CASES else from_edge(name)
    return _cache[name]


# ---- the oracle, marker by marker -----------------------------------------------------------------
def _oracle(case_or_n, start, joseph):
    n = case_or_n if isinstance(case_or_n, int) else case_or_n.n_landmarks
    ref = orc.OracleEKF(n_landmarks=n, joseph=joseph)
    if start is not None:
        x, S, tmo, cnt = start
        ref.set(x, S, tmo, x[:3], cnt)
    return ref


def _marker_event(ref, n_landmarks, lid, rx, ry):
    """Corrects marker (lid, rx, ry) on the oracle → (rc, kind of rare event or None, the margin
    |.| of the step's angles from normalize_angle_near's limit)."""
    x = ref.get(sigma=False)[0]
    if lid < 0 or lid >= n_landmarks:
        return -2, "range", math.inf
    lx, ly = x[3 + 2 * lid], x[4 + 2 * lid]
    kind = None
    margin = math.inf
    if lx == 0.0 and ly == 0.0:
        kind = "first"
    else:
        braw = math.atan2(ly - x[2], lx - x[1]) - x[0]
        margin = min(abs(abs(braw + math.pi) - FIVE_PI), abs(abs(x[0] + math.pi) - FIVE_PI))
        if abs(braw + math.pi) >= FIVE_PI or abs(x[0] + math.pi) >= FIVE_PI:
            kind = "angle"
    rc = ref.correct(lid, rx, ry)
    if rc == es.NUMERIC and kind is None:
        kind = "numeric"
    return rc, kind, margin


def locate(case: Case, joseph=False):
    """The oracle through the case, marker by marker → dict(events = {(message, chunk): (position
    of the chunk's first rare event, its kind)}, all_events = [(message, marker, kind)], rcs [T]
    (the first nonzero code of each message), poses [T, 3], state, sigma, tmo, counter, margin)."""
    e = case.edge
    ref = _oracle(case, case.start, joseph)
    T = e.n_messages
    events, every = {}, []
    rcs, poses, margin = np.zeros(T, np.int32), np.zeros((T, 3)), math.inf
    for t in range(T):
        ref.set_odom(e.odom[t])
        ref.predict()
        for i in range(int(e.count[t])):
            rc, kind, mg = _marker_event(ref, e.n_landmarks, int(e.ids[t, i]), *e.rel[t, i])
            margin = min(margin, mg)
            if rc and not rcs[t]:
                rcs[t] = rc
            if kind is not None:
                every.append((t, i, kind))
                events.setdefault((t, i // CHUNK), (i % CHUNK, kind))
        ref.posterior()
        poses[t] = ref.get(sigma=False)[0][:3]
    x, S, tmo, cnt = ref.get()
    return dict(events=events, all_events=every, rcs=rcs, poses=poses, state=x, sigma=S, tmo=tmo,
                counter=cnt, margin=margin)


def expected_counts(case: Case, events) -> np.ndarray:
    """[T, 2]: the corrections of each message the lean and the generic program run — a chunk's
    markers before its first event, and the rest."""
    e = case.edge
    out = np.zeros((e.n_messages, 2), np.int64)
    for t in range(e.n_messages):
        c = int(e.count[t])
        for k in range((c + CHUNK - 1) // CHUNK):
            m = min(CHUNK, c - k * CHUNK)
            lean = events[t, k][0] if (t, k) in events else m
            out[t] += (lean, m - lean)
    return out


def locate_heading_state(hs, joseph=False):
    """edge_scenarios.heading_state's corrections (ekf_correct per marker: each its own chunk, no
    predict) → (kinds [m]: each correction's rare event or None, the angles' margin)."""
    x0, S0, tmo0, od, ids, rel = hs
    N = (x0.shape[0] - 3) // 2
    ref = _oracle(N, (x0, S0, tmo0, 0), joseph)
    ref.set_odom(od)
    kinds, margin = [], math.inf
    for lid, (rx, ry) in zip(ids, rel):
        rc, kind, mg = _marker_event(ref, N, int(lid), rx, ry)
        assert rc == 0
        kinds.append(kind)
        margin = min(margin, mg)
    return kinds, margin
