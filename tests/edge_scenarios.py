"""Inputs that drive the correction kernels' generic ("rare") paths, and their oracle runs.

Every correction kernel runs the common case branch-free and sends everything else to one
wave-uniform fallback: a singular or non-finite innovation covariance S (the marker is skipped,
EKF_FLAG_NUMERIC; the oracle's correct_slot returns -4), a bearing or innovation outside
normalize_angle_near's range, a heading beyond it. The builders here produce documented inputs that
reach those branches:

* Z: a first sighting at range 0 (rel = (0, 0)): the landmark lands on the robot, H is NaN
  (slam.cpp:241-249) and arma::inv throws in the reference; the oracle skips the correction and
  keeps the landmark where the first sighting put it.
* H: odometry whose heading lies far outside (-pi, pi] (geom.hpp compose does not wrap): the
  predict's normalize_angle takes its generic fmod branch (|a + pi| >= 5 pi) and hands the chain
  a heading in (-pi, pi]. The chain's own fallbacks for a bearing and an updated heading beyond
  normalize_angle_near's range run when there is no predict: heading_state loads such a heading
  with ekf_set_state and corrects with no predict pending. (The innovation's fallback cannot be
  reached with finite input: z1 is an atan2 and zhat1 is normalised by then, so |z1 - zhat1| <=
  2 pi; the non-finite innovations of Z do take that branch, into the skip.)
* S: a landmark straight behind the robot, bearings alternating about the +-pi seam, and a heading
  that every correction pushes across the seam.
* A: a range-0 marker under unknown association (the phantom landmark is committed, the
  correction skipped).

tests/test_edge_scenarios.py pins each scenario's properties with the oracle alone (both of its
arithmetic modes), so that the GPU tests that replay them can neither pass vacuously nor fail
through ill-conditioning. Odometry is integrated by the oracle's own DiffDrive, on the CPU and in
the GPU tests alike: both see the same bits.
"""
from __future__ import annotations

import json
import math
import os
from dataclasses import dataclass

import numpy as np

import orc
from pyekf import synth

GATE = 2.0
NUMERIC = -4  # orc correct_slot's skip; EKF_E_NUMERIC
# (pose, state, Σ) bounds of the GPU comparisons, none new: test_gpu_parity.py's fp64 bounds for the
# known-id scenarios, test_gpu_scale.py's populated-map bounds for the association ones, and its
# N = 256 survey test's fp32 bounds. The oracle's two modes must agree ten times tighter than the
# fp64 bounds on every scenario (test_edge_scenarios.py).
KNOWN_TOL = (1e-8, 1e-8, 1e-8)
ASSOC_TOL = (1e-8, 5e-8, 1e-7)
F32_TOL = (5e-6, 1e-5, 5e-5)


@dataclass
class Edge:
    name: str
    n_landmarks: int
    count: np.ndarray      # [T]
    ids: np.ndarray        # [T, M]
    actions: np.ndarray    # [T, M]
    rel: np.ndarray        # [T, M, 2]
    odom: np.ndarray       # [T, 3] t_odom_robot at each message (theta, x, y)
    assoc: bool = False
    skips: tuple = ()      # messages the oracle must answer with -4 (every other one with 0)
    zeros: tuple = ()      # (message, position) of each rel = (0, 0) marker

    @property
    def n_messages(self) -> int:
        return int(self.count.shape[0])


def oracle_odometry(sc) -> np.ndarray:
    """t_odom_robot at each message of a synth.Scenario by the oracle's DiffDrive (fkin per tick)."""
    dd = orc.DiffDrive(sc.track, sc.radius)
    out = np.zeros((sc.n_messages, 3))
    for t in range(sc.n_messages):
        for k in range(sc.wheel.shape[1]):
            p = dd.fkin(sc.wheel[t, k, 0], sc.wheel[t, k, 1])
        out[t] = p
    return out


def _edge(name, sc, theta=None, **kw) -> Edge:
    odom = oracle_odometry(sc)
    if theta is not None:
        odom[:, 0] += theta
    return Edge(name, sc.n_landmarks, sc.count.copy(), sc.ids.copy(), sc.actions.copy(),
                sc.rel.copy(), odom, **kw)


def _zero(e: Edge, t: int, pos: int, lid: int | None):
    e.rel[t, pos] = 0.0
    if lid is not None:
        e.ids[t, pos] = lid
    e.zeros += ((t, pos),)
    if t not in e.skips:
        e.skips += (t,)


# ---- Z / H: known ids -----------------------------------------------------------------------------
def _base(n_markers=12):
    """12 (16, 20) landmarks, all in range of the unit circle, in a filter with 8 (4, 4) spare slots:
    every message reports ids 0..n_markers-1; the spare ids are never reported."""
    n = {12: 20, 16: 20, 20: 24}[n_markers]
    return synth.make_scenario(n, synth.random_landmarks(n_markers, seed=7), 12,
                               max_markers=n_markers, seed=8)


def theta_offset(kind: str, T: int) -> np.ndarray:
    """+25: the robot spun four times before its first message; +20 / -25: a jump from message 5."""
    th = np.zeros(T)
    if kind == "p25":
        th[:] = 25.0
    elif kind == "p20":
        th[5:] = 20.0
    elif kind == "m25":
        th[5:] = -25.0
    else:
        raise ValueError(kind)
    return th


def clean() -> Edge:
    return _edge("clean", _base())


def zero_range(p: int, n_markers: int = 12, theta: str | None = None) -> Edge:
    """Z: position p of messages 0 and 6 becomes a first sighting of a spare id (the last, then the
    one before) at rel = (0, 0). The spare ids are never reported again (a range-0 landmark that
    later messages re-observe makes the oracle's own two modes differ by 1.7e-7)."""
    sc = _base(n_markers)
    assert np.all(sc.count == n_markers) and p < n_markers
    name = f"Z{n_markers}_p{p}" + (f"_{theta}" if theta else "")
    e = _edge(name, sc, None if theta is None else theta_offset(theta, sc.n_messages))
    _zero(e, 0, p, sc.n_landmarks - 1)
    _zero(e, 6, p, sc.n_landmarks - 2)
    return e


def heading(kind: str) -> Edge:
    sc = _base()
    return _edge("H_" + kind, sc, theta_offset(kind, sc.n_messages))


def heading_state(turns: int):
    """H without a predict: the oracle's state after the clean drive's first 6 messages with
    `turns` whole turns added to the heading (theta = theta6 + 2 pi turns, the same orientation),
    to be loaded with ekf_set_state and corrected by message 6's markers through ekf_correct with
    no predict pending. The chain then starts from a heading outside (-pi, pi]: the bearing
    atan2(..) - theta and the updated heading both lie beyond normalize_angle_near's |a + pi| <
    5 pi, and its generic fallbacks run. → (x0, S0, tmo0, odom6, ids6, rel6)."""
    e = get("clean")
    ref = orc.OracleEKF(n_landmarks=e.n_landmarks)
    for t in range(6):
        ref.set_odom(e.odom[t])
        c = int(e.count[t])
        assert ref.fake_sensor_cb(e.ids[t, :c], e.actions[t, :c], e.rel[t, :c]) == 0
    x, S, tmo, _ = ref.get()
    x[0] += 2.0 * math.pi * turns
    c = int(e.count[6])
    return x, S, tmo, e.odom[6], e.ids[6, :c], e.rel[6, :c]


def run_heading_state(hs, literal=False, joseph=False):
    """The oracle from heading_state's state: correct per marker (no predict), posterior →
    (state, sigma, tmo, pose after each correction [m, 3])."""
    x0, S0, tmo0, od, ids, rel = hs
    ref = orc.OracleEKF(n_landmarks=(x0.shape[0] - 3) // 2, literal=literal, joseph=joseph)
    ref.set(x0, S0, tmo0, x0[:3], 0)
    ref.set_odom(od)
    th = []
    for lid, (rx, ry) in zip(ids, rel):
        assert ref.correct(lid, rx, ry) == 0
        th.append(ref.get(sigma=False)[0][:3])
    ref.posterior()
    x, S, tmo, _ = ref.get()
    return x, S, tmo, np.array(th)


# ---- S: the +-pi seam -----------------------------------------------------------------------------
def seam(T: int = 10) -> Edge:
    """A robot creeping along -x with its heading 5e-5 short of pi, and landmark 3 straight behind
    it: its measured bearing alternates between -(pi - 1e-3) and +(pi - 1e-3), so its raw innovation
    is +-2 pi every other message, and the 2e-3 rad it moves theta by each time carries theta across
    the seam and back."""
    N = 6
    lm = {1: (-1.2, 0.9), 4: (0.6, -1.1), 0: (-0.4, -0.8)}
    ids = np.array([1, 3, 4, 0], np.int32)
    M = ids.size
    rng = np.random.default_rng(5)
    rel = np.zeros((T, M, 2))
    odom = np.zeros((T, 3))
    for t in range(T):
        th, x, y = math.pi - 5e-5, -0.02 * t, 0.0        # the true pose = the odometry
        odom[t] = (th, x, y)
        for i, lid in enumerate(ids):
            if lid == 3:
                b = (math.pi - 1e-3) * (-1.0 if t % 2 == 0 else 1.0)
                r = 1.5 + 0.02 * t
                rel[t, i] = (r * math.cos(b), r * math.sin(b))
            else:
                dx, dy = lm[int(lid)][0] - x, lm[int(lid)][1] - y
                c, s = math.cos(th), math.sin(th)
                rel[t, i] = (c * dx + s * dy, -s * dx + c * dy)
                rel[t, i] += rng.normal(0.0, 1e-3, 2)
    return Edge("S_seam", N, np.full(T, M, np.int32), np.repeat(ids[None], T, 0),
                np.zeros((T, M), np.int32), rel, odom)


def seam_trace(e: Edge):
    """The oracle (structured) through S by predict / correct / posterior: per correction the raw
    innovation z1 - zhat1 before normalisation and theta before and after."""
    ref = orc.OracleEKF(n_landmarks=e.n_landmarks)
    raw, before, after = [], [], []
    for t in range(e.n_messages):
        ref.set_odom(e.odom[t])
        ref.predict()
        for i in range(int(e.count[t])):
            x = ref.get(sigma=False)[0]
            lid = int(e.ids[t, i])
            rx, ry = e.rel[t, i]
            zb = math.atan2(ry, rx)
            lx, ly = x[3 + 2 * lid], x[4 + 2 * lid]
            if lx == 0.0 and ly == 0.0:   # first sighting: zhat is the measurement (slam.cpp:213)
                zr = math.hypot(rx, ry)
                lx, ly = x[1] + zr * math.cos(zb + x[0]), x[2] + zr * math.sin(zb + x[0])
            zhat = orc.normalize_angle(math.atan2(ly - x[2], lx - x[1]) - x[0])
            raw.append(zb - zhat)
            before.append(x[0])
            assert ref.correct(lid, rx, ry) == 0
            after.append(ref.get(sigma=False)[0][0])
        ref.posterior()
    return np.array(raw), np.array(before), np.array(after)


# ---- A: unknown association -----------------------------------------------------------------------
def assoc_zero(N: int, pos: int | str, theta: str | None = None, seed: int | None = None,
               also=()) -> Edge:
    """A: shuffled markers without ids; the last message's marker at `pos` ("last": its last) is
    rel = (0, 0); `also`: further zeros as (message, position), negative indices from the end.
    (A range-0 marker many messages before the end spreads the oracle's modes by 5.9e-7.)
    Both drives are re-seeded, each with one seed for all its variants. N = 20 uses 14: with seed 8
    the oracle's two modes differ by 5.1e-9 in the state at position 3 (the marker that associates
    with the phantom corrects against a landmark 1e-3 m from the robot), over the tenth of the
    5e-8 bound that the pin allows; seed 14 gives at most 3.0e-9 in every variant. N = 130 uses 18:
    with seed 12 the Joseph form's two modes differ by 2.4e-8 in the state at position 3 and by
    1.0e-9 in the poses with the +25 rad heading; seed 18 stays under 2e-9 / 4e-10."""
    if N == 20:
        sc = synth.make_scenario(20, synth.random_landmarks(12, seed=7), 10, max_markers=16,
                                 seed=14 if seed is None else seed, shuffle=True)
    elif N == 130:
        sc = synth.make_scenario(130, synth.random_landmarks(100, seed=11), 10, max_markers=16,
                                 seed=18 if seed is None else seed, shuffle=True)
    else:
        raise ValueError(N)
    T = sc.n_messages
    name = f"A{N}_{pos}" + (f"_{theta}" if theta else "")
    e = _edge(name, sc, None if theta is None else theta_offset(theta, T), assoc=True)
    e.ids[:] = -1
    if pos is not None:
        _zero(e, T - 1, int(e.count[T - 1]) - 1 if pos == "last" else int(pos), None)
    for t, p in also:
        t %= T
        _zero(e, t, p % int(e.count[t]), None)
    e.skips = tuple(sorted(e.skips))
    return e


# ---- association on the last slot of the last workgroup ----------------------------------------------
# N → the landmark of populated(N, 6, shuffle=True) that is relabelled to slot N - 1: of those the
# circle messages sight, the one first sighted latest that the oracle then commits as new (on these
# dense maps a landmark at the edge of the sensed set can fall inside a mapped neighbour's gate).
# Pinned by tests/test_edge_scenarios.py.
LAST_SLOT = {63: 43, 65: 2, 127: 19, 129: 111}


def last_slot_scenario(N: int):
    """populated(N, 6, shuffle=True) with landmark ids LAST_SLOT[N] and N - 1 exchanged."""
    sc = synth.populated(N, 6, shuffle=True)
    perm = np.arange(N, dtype=np.int32)
    perm[LAST_SLOT[N]], perm[N - 1] = N - 1, LAST_SLOT[N]
    ids = np.where(sc.ids >= 0, perm[np.maximum(sc.ids, 0)], -1).astype(np.int32)
    return synth.Scenario(sc.n_landmarks, sc.landmarks, sc.wheel, ids, sc.actions, sc.rel,
                          sc.count, sc.truth, sc.track, sc.radius, sc.n_warm)


def forget_last(x, S, init_var=10e6):
    """The last landmark slot back to the prior (slam.cpp:127-132; `init_var`: the filter's, by
    default the reference's), in place."""
    k = x.shape[0] - 2
    x[k:] = 0.0
    S[k:, :] = 0.0
    S[:, k:] = 0.0
    S[k, k] = S[k + 1, k + 1] = init_var


# ---- the oracle -----------------------------------------------------------------------------------
def run_oracle(e: Edge, literal=False, joseph=False, **params):
    """The oracle (`params`: q_noise, r_noise, init_var, mah_gate where they are not the defaults)
    through every message of `e` → rcs [T], poses [T, 3], final state / sigma / tmo /
    counter, the heading of t_map_odom * t_odom_robot before slam.cpp:186 normalises it (raw_theta
    [T]) and, under association, decisions j / new [T, M] and each marker's smallest existing
    Mahalanobis distance dmin [T, M] (NaN padded)."""
    ref = orc.OracleEKF(n_landmarks=e.n_landmarks, literal=literal, joseph=joseph, **params)
    T, M = e.ids.shape
    rcs = np.zeros(T, np.int32)
    poses = np.zeros((T, 3))
    aj = np.full((T, M), -1, np.int32)
    an = np.zeros((T, M), np.int32)
    dmin = np.full((T, M), np.nan)
    cnts = np.zeros(T, np.int64)
    raw = np.zeros(T)
    for t in range(T):
        c = int(e.count[t])
        raw[t] = ref.get(sigma=False)[2][0] + e.odom[t, 0]
        ref.set_odom(e.odom[t])
        if e.assoc:
            rcs[t], aj[t, :c], an[t, :c], dmin[t, :c] = ref.sensor_cb_dmin(e.rel[t, :c])
        else:
            rcs[t] = ref.fake_sensor_cb(e.ids[t, :c], e.actions[t, :c], e.rel[t, :c])
        x, _, _, cnts[t] = ref.get(sigma=False)
        poses[t] = x[:3]
    x, S, tmo, cnt = ref.get()
    return dict(rcs=rcs, poses=poses, state=x, sigma=S, tmo=tmo, counter=cnt, assoc_j=aj,
                assoc_new=an, dmin=dmin, counters=cnts, raw_theta=raw)


def expected_rcs(e: Edge) -> np.ndarray:
    rc = np.zeros(e.n_messages, np.int32)
    rc[list(e.skips)] = NUMERIC
    return rc


KNOWN = {
    "Z12_p0": lambda: zero_range(0),
    "Z12_p3": lambda: zero_range(3),
    "Z12_p11": lambda: zero_range(11),
    "Z16_p15": lambda: zero_range(15, 16),
    "Z20_p15": lambda: zero_range(15, 20),
    "Z20_p16": lambda: zero_range(16, 20),
    "H_p25": lambda: heading("p25"),
    "H_p20": lambda: heading("p20"),
    "H_m25": lambda: heading("m25"),
    "Z12_p3_p20": lambda: zero_range(3, theta="p20"),
    "S_seam": seam,
}
ASSOC = {
    "A20_3": lambda: assoc_zero(20, 3),
    "A20_last": lambda: assoc_zero(20, "last"),
    "A130_3": lambda: assoc_zero(130, 3),
    "A130_last": lambda: assoc_zero(130, "last"),
    "A20_3_p25": lambda: assoc_zero(20, 3, "p25"),
    "A130_last_p25": lambda: assoc_zero(130, "last", "p25"),
}
# several skips in one run, for the return codes of the synchronous forms: a zero closing each of
# the last two messages; two zeros in the last message; a zero closing the message before the last
# and none in the last
ASSOC_MULTI = {
    "A20_two_msgs": lambda: assoc_zero(20, "last", also=((-2, -1),)),
    "A20_two_same": lambda: assoc_zero(20, 3, also=((-1, -1),)),
    "A20_zero_then_clean": lambda: assoc_zero(20, None, also=((-2, -1),)),
    # ... the same with three workgroups. The last message's first marker associates with the
    # landmark the skipped marker left at its prior variance: with fp32 Σ that correction cancels
    # 1e7 - (1e7 - d) like a first sighting (at N = 20 in a chunk that commits nothing)
    "A130_zero_then_clean": lambda: assoc_zero(130, None, also=((-2, -1),)),
}
_cache: dict = {}


def get(name: str) -> Edge:
    """The named scenario, built once per process (treat it as read-only)."""
    if name not in _cache:
        _cache[name] = clean() if name == "clean" else {**KNOWN, **ASSOC, **ASSOC_MULTI}[name]()
    return _cache[name]


def write_errors(section, errors):
    """One module's measured errors as its section of edge_errors.json (the section is rewritten
    whole, the other module's kept), beside test_gpu_scale.py's scale_errors.json: the directory
    is the one that module defines."""
    from test_gpu_scale import errors_dir
    path = os.path.join(errors_dir(), "edge_errors.json")
    try:
        with open(path) as fh:
            doc = json.load(fh)
    except (OSError, ValueError):
        doc = {}
    doc[section] = errors
    with open(path, "w") as fh:
        json.dump(doc, fh, indent=1)
