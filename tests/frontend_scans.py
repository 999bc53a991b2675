"""Scans and point clusters that drive the landmark front-end's edge paths, and their oracle runs.

The front-end's kernels (ekf-slam_amd/csrc/lm_kernels.hip) have paths that ordinary scans do not
reach. The families here are built to reach them:

* ``dense_ring``: 2048 beams, rings of 90 to 120 cylinders, 155 to 240 candidates per scan with
  passing (cylinder) and failing (wall) candidates alternating: k_markers' loop over 64-candidate
  chunks carries its id and slot bases across up to four iterations.
* ``size_limits``: clusters of exactly 3, 4, 39 and 40 points (the gate is 3 < n < 40), each as an
  ordinary cluster and as cluster 0 merged from the scan's two ends.
* ``chunk_edges``: one scene turned by whole beams, so that the breaks pass over the 64-beam chunk
  edges of the ballot compaction and over beams 1 and B − 1.
* ``odd_beams``: beam counts around the wave size, not multiples of 8, and down to 2.
* ``degenerate``: every beam a break, exactly one break (merged and not), non-finite ranges at the
  scan's two ends, an all-NaN scan, and rooms with no break at all.

``fit_arcs`` / ``triples`` are the seeded point clusters of the direct fit tests.

Every case keeps the oracle away from its decision thresholds (``margin_violations``), so that a
last-bit difference in sincos or acos cannot legitimately flip a decision, and keeps every fitted
cluster out of the noise band in which the reference's Hyper fit is itself ill-determined in double
precision ("The ill-determined band"). tests/test_frontend_scans.py pins all of
this with the oracle alone; tests/test_gpu_landmarks_edges.py runs the cases on the GPU.
"""
from __future__ import annotations

import functools
import math
from dataclasses import dataclass

import numpy as np

import landmarks_numpy as L

THRESHOLD = L.CLUSTER_THRESHOLD
ANGLE_MIN_ALT = float(np.float32(-0.01))   # the second per-scan angle_min of the batches
BAND = (1e-12, 3e-9)                       # residual rms in which the Hyper fit is ill-determined
FIT_SIGMAS = (1e-5, 1e-6, 1e-7, 1e-8, 1e-13, 1e-14, 0.0)
ODD_BEAMS = (63, 64, 65, 127, 128, 129, 2047)
RING_SPECS = ((100, 1.0, 0.02), (120, 1.2, 0.02), (90, 0.9, 0.025))
# (candidates, markers, highest id) of the oracle on each dense ring
RING_COUNTS = ((200, 99, 98), (240, 119, 118), (155, 89, 88), (159, 49, 97))
# the scene that chunk_edges turns and odd_beams resamples
SCENE = ((1.44, 0.54, 0.15), (-0.9, -1.26, 0.15), (0.18, 1.62, 0.12))


def default_inc(n_beams):
    return float(np.float32(2.0 * math.pi / n_beams))


@dataclass(frozen=True, eq=False)
class Case:
    name: str
    ranges: np.ndarray       # float32 [B], read-only
    angle_min: float
    angle_inc: float

    @property
    def n_beams(self):
        return int(self.ranges.shape[0])


def _case(name, ranges, angle_min=0.0, angle_inc=None):
    r = np.array(ranges, dtype=np.float32)
    r.setflags(write=False)
    return Case(name, r, float(angle_min), default_inc(len(r)) if angle_inc is None else angle_inc)


# ------------------------------------------------------------------------------------ families

@functools.lru_cache(maxsize=None)
def dense_ring():
    out = []
    for n, d, r in RING_SPECS:
        circles = [(d * math.cos(2.0 * math.pi * k / n + 0.01),
                    d * math.sin(2.0 * math.pi * k / n + 0.01), r) for k in range(n)]
        out.append(_case(f"dense_ring_{n}", L.synthetic_scan((0.0, 0.0, 0.0), circles,
                                                             n_beams=2048)))
    # every second cylinder beyond the 2 m publish range: circles that take an id and no marker
    # slot, so that ids and slots differ
    n, r = 100, 0.03
    circles = [((1.0 if k % 2 == 0 else 2.2) * math.cos(2.0 * math.pi * k / n + 0.01),
                (1.0 if k % 2 == 0 else 2.2) * math.sin(2.0 * math.pi * k / n + 0.01), r)
               for k in range(n)]
    out.append(_case("dense_ring_far", L.synthetic_scan((0.0, 0.0, 0.0), circles, n_beams=2048)))
    return tuple(out)


# size_limits: clusters of exactly 3, 4, 39 and 40 points in 360-beam scans. "plain": a cylinder abeam
# of the lidar at pose (0, 0, 0), an ordinary cluster; a cluster loses the first beam that hits its
# cylinder (the breaking point is dropped, landmarks.cpp:81-86). "merged": cluster 0, made of the
# scan's first beams and its last ones.
def _abeam(d, r, half_beam):
    a = math.pi / 2.0 + (math.pi / 360.0 if half_beam else 0.0)
    return (-L.LIDAR_X_OFFSET + d * math.cos(a), d * math.sin(a), r)


# A cylinder on a beam's axis is hit by 2m + 1 beams and keeps 2m of them: the odd sizes sit half a
# beam off the axis. Every one of these clusters passes check_circle, so that the size gate alone
# decides whether it becomes a marker.
SIZE_SCENES = {3: _abeam(0.96, 0.03, True), 4: _abeam(1.0, 0.045, False),
               39: _abeam(0.292, 0.1, True), 40: _abeam(0.2795, 0.1, False)}
# merged sizes: (beams of the circle at the scan's start, at its end)
SIZE_MERGED = {3: (2, 1), 4: (2, 2), 39: (20, 19), 40: (20, 20)}


def _merged_circle(n_first, n_last, B=360):
    """Ranges written directly: a room of 3 m, and 0.28 m ahead of the lidar a circle of radius
    0.097 m of which beams 0 … n_first − 1 see the near side and the last n_last beams the far side
    (the beam before those sits next to the first of them: the breaking point, dropped). The scan
    closes on itself, so
    cluster 0 is the two runs: its first point (beam 0, near) and its last (beam B − 1, far) are all
    but a diameter apart and every other point sees that chord under about π/2: unlike a cylinder
    ahead of a real lidar, whose cluster 0 has its end points next to each other and fails
    check_circle at any size, this cluster passes it, and the size gate decides. A ripple of 20 µm
    keeps the fit clear of the ill-determined band."""
    D, r = 0.28, 0.097
    out = np.full(B, 3.0)
    for i in list(range(n_first)) + list(range(B - n_last, B)):
        a = (i if i < n_first else i - B) * 2.0 * math.pi / B
        root = math.sqrt(r * r - (D * math.sin(a)) ** 2)
        out[i] = D * math.cos(a) + (-root if i < n_first else root) + 2e-5 * math.sin(7.0 * i)
    out[B - n_last - 1] = out[B - n_last]
    return out


@functools.lru_cache(maxsize=None)
def size_limits():
    plain = [_case(f"size_plain_{n}", L.synthetic_scan((0.0, 0.0, 0.0), [c]))
             for n, c in SIZE_SCENES.items()]
    merged = [_case(f"size_merged_{n}", _merged_circle(*runs)) for n, runs in SIZE_MERGED.items()]
    return tuple(plain + merged)


@functools.lru_cache(maxsize=None)
def chunk_edges():
    return tuple(_case(f"chunk_edges_{k}",
                       L.synthetic_scan((k * 2.0 * math.pi / 360.0, 0.0, 0.0), list(SCENE)))
                 for k in range(64))


@functools.lru_cache(maxsize=None)
def odd_beams():
    out = []
    for B in ODD_BEAMS:
        # few beams: a small arena and fat, near cylinders, so that clusters of ≥ 4 beams exist
        # (many beams: thin ones, so that their clusters stay below 40 points)
        if B < 256:
            circles, arena = [(0.62, 0.2, 0.18), (-0.4, -0.6, 0.18), (0.05, 0.75, 0.16)], (2.4, 2.0)
        else:
            circles, arena = [(x, y, r / 3.0) for x, y, r in SCENE], (10.0, 5.0)
        pose = (0.05 if B < 256 else 0.3, 0.0, 0.0)
        out.append(_case(f"odd_beams_{B}", L.synthetic_scan(pose, circles, arena=arena, n_beams=B)))
    # written directly, 0.01 rad between beams (at 2π/B the beams of so short a scan point in
    # opposite directions and every one of them is a break)
    for name, r in (("2_break", [0.5, 3.0]),                    # one break, count 0
                    ("2_room", [0.5, 0.5]),                     # no break
                    ("3_break", [0.5, 0.5, 3.0]),               # break at B − 1, not merged
                    ("3_room", [0.5, 0.5, 0.5]),
                    ("5_break", [0.5, 0.5, 3.0, 0.5, 0.5]),     # breaks at 2 and 3, merged: n = 3
                    ("5_first", [0.5, 3.0, 3.0, 3.0, 3.0]),     # break at i = 1, not merged: n = 3
                    ("5_room", [0.5, 0.5, 0.5, 0.5, 0.5])):
        out.append(_case(f"odd_beams_{name}", r, angle_inc=float(np.float32(0.01))))
    return tuple(out)


def _base_scan():
    return np.array(L.synthetic_scan((0.2, 0.1, -0.05), list(SCENE)))


@functools.lru_cache(maxsize=None)
def degenerate():
    out = []
    for B in (2048, 65):   # every beam a break; B = 65 closes on itself (both ends at 0.5 m)
        r = np.where(np.arange(B) % 2 == 0, 0.5, 3.0)
        out.append(_case(f"degenerate_alternating_{B}", r))
    room = np.full(360, 1.0)
    r = room.copy()
    r[180] = 3.0           # a far beam mid-scan: breaks at 180 and 181, the two ends merge
    out.append(_case("degenerate_far_beam_mid", r))
    r = room.copy()
    r[359] = 3.0           # a far beam at B − 1: exactly one break, not merged
    out.append(_case("degenerate_one_break_open", r))
    # a spiral with one step: exactly one break (at beam 180), and the scan closes on itself
    i = np.arange(360)
    r = np.where(i < 180, 1.0 + 0.15 * i / 179.0, 0.85 + 0.15 * (i - 180) / 180.0)
    out.append(_case("degenerate_one_break_merged", r))
    for name, idx, v in (("nan_first", [0], np.nan), ("nan_last", [359], np.nan),
                         ("inf_ends", [0, 359], np.inf)):
        r = _base_scan()
        r[idx] = v
        out.append(_case(f"degenerate_{name}", r))
    out.append(_case("degenerate_all_nan", np.full(360, np.nan)))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def rooms():
    """360-beam scans without a break (the reference throws: LM_NO_BREAK), for the batches."""
    i = np.arange(360)
    return (_case("room_round", np.full(360, 1.0)),
            _case("room_near", np.full(360, 0.3)),
            _case("room_wavy", 1.5 + 0.2 * np.sin(i * 2.0 * math.pi / 360.0)))


FAMILIES = {"dense_ring": dense_ring, "size_limits": size_limits, "chunk_edges": chunk_edges,
            "odd_beams": odd_beams, "degenerate": degenerate}


def all_cases():
    return tuple(c for f in FAMILIES.values() for c in f())


@functools.lru_cache(maxsize=None)
def batch_cases():
    """130 scans of 360 beams: the size limits, the turned scene and no-break rooms interleaved,
    with angle_min alternating between 0 and float32(−0.01)."""
    pool = iter(list(size_limits()) + list(chunk_edges()) + list(size_limits()) * 5)
    rm = rooms()
    out = []
    for s in range(130):
        c = rm[(s // 7) % len(rm)] if s % 7 == 3 else next(pool)
        out.append(Case(c.name, c.ranges, ANGLE_MIN_ALT if s % 2 else 0.0, c.angle_inc))
    return tuple(out)


def small_batch():
    """Three scans of 65 beams (the handle-reuse sequence)."""
    c = {x.name: x for x in odd_beams() + degenerate()}
    return (c["odd_beams_65"], c["degenerate_alternating_65"],
            Case("odd_beams_65", c["odd_beams_65"].ranges, ANGLE_MIN_ALT, c["odd_beams_65"].angle_inc))


# ------------------------------------------------------------------------------------- oracle

_ORACLE: dict = {}


def oracle(case):
    """laser_callback of the case: a tuple of (id, x, y, r), or None where the reference throws.
    Computed once per (scan, angles)."""
    key = (case.name, case.angle_min, case.angle_inc)
    if key not in _ORACLE:
        m = L.laser_callback(case.ranges, case.angle_min, case.angle_inc)
        _ORACLE[key] = None if m is None else tuple(m)
    return _ORACLE[key]


def expected_rows(cases, max_markers):
    """(counts [S], ids [S, max_markers], xyr [S, max_markers, 3], valid [S, max_markers]) as
    lm_detect reports the oracle's results: the count is the full count, the rows its first
    ``max_markers`` markers."""
    S = len(cases)
    cnt = np.zeros(S, np.int32)
    ids = np.zeros((S, max_markers), np.int32)
    xyr = np.zeros((S, max_markers, 3))
    valid = np.zeros((S, max_markers), bool)
    for s, c in enumerate(cases):
        m = oracle(c)
        cnt[s] = -1 if m is None else len(m)
        for i, (k, x, y, r) in enumerate((m or ())[:max_markers]):
            ids[s, i], xyr[s, i], valid[s, i] = k, (x, y, r), True
    return cnt, ids, xyr, valid


def break_indices(case):
    """Beams i ≥ 1 farther than the threshold from beam i − 1 (or not comparable to it)."""
    p = L.scan_points(case.ranges, case.angle_min, case.angle_inc)
    return [i for i in range(1, len(p)) if not L._dist(p[i], p[i - 1]) <= THRESHOLD]


def cluster_sizes(case):
    """(sizes of the oracle's clusters, whether the scan's last run was merged into cluster 0)."""
    cl = L.get_clusters(case.ranges, case.angle_min, case.angle_inc)
    if cl is None:
        return None, False
    nb = len(break_indices(case))
    return [len(c) for c in cl], len(cl) == nb


def circle_stats(cluster):
    """(std, mean) of check_circle's inscribed angles, with the cosine clipped to [−1, 1]: three
    collinear points put it at −1 ± an ulp, where acos is NaN or π by the last bit."""
    p0, p1 = cluster[0], cluster[-1]
    c = L._dist(p0, p1)
    ang = []
    for q in cluster[1:-1]:
        a, b = L._dist(p0, q), L._dist(p1, q)
        with np.errstate(all="ignore"):
            x = np.float64(c * c - a * a - b * b) / np.float64(-2.0 * a * b)
        ang.append(float(np.arccos(np.clip(x, -1.0, 1.0))))
    ang = np.array(ang)
    with np.errstate(all="ignore"):
        return (float(np.std(ang, ddof=1)) if len(ang) > 1 else 0.0), float(np.mean(ang))


def residual_rms(cluster, fit):
    P = np.asarray(cluster, dtype=np.float64).reshape(-1, 2)
    res = np.hypot(P[:, 0] - fit[0], P[:, 1] - fit[1]) - fit[2]
    return float(np.sqrt(np.mean(res ** 2)))


def in_band(cluster, fit=None):
    rms = residual_rms(cluster, L.fit_circle(cluster) if fit is None else fit)
    return BAND[0] < rms < BAND[1]


def margin_violations(case):
    """The margins the case breaks (an empty list: none). See the module docstring."""
    bad = []
    p = L.scan_points(case.ranges, case.angle_min, case.angle_inc)
    B = len(p)
    for i in range(B):   # i = 0: the closing distance of the merge test
        d = L._dist(p[i], p[i - 1])
        if math.isfinite(d) and abs(d - THRESHOLD) <= 1e-9:
            bad.append(f"distance {i - 1}→{i} = {d!r}")
    cl = L.get_clusters(case.ranges, case.angle_min, case.angle_inc)
    for k, c in enumerate(cl or []):
        if not 3 < len(c) < 40:
            continue
        sd, mn = circle_stats(c)
        if not (math.isfinite(sd) and math.isfinite(mn)):
            continue   # a repeated point: NaN on both sides, not a circle
        if bool(sd < 0.2 and 1.3 < mn < 2.6) != L.check_circle(c):
            bad.append(f"cluster {k}: check_circle decided by the clip")
        if abs(sd - 0.2) <= 1e-6 or abs(mn - 1.3) <= 1e-6 or abs(mn - 2.6) <= 1e-6:
            bad.append(f"cluster {k}: std {sd!r} mean {mn!r}")
        if not L.check_circle(c):
            continue
        f = L.fit_circle(c)
        if not abs(f[2] - L.MAX_RADIUS) > 1e-6:
            bad.append(f"cluster {k}: R {f[2]!r}")
        if not abs(math.hypot(f[0], f[1]) - L.MAX_RANGE) > 1e-6:
            bad.append(f"cluster {k}: centre distance {math.hypot(f[0], f[1])!r}")
        rms = residual_rms(c, f)
        if BAND[0] < rms < BAND[1]:
            bad.append(f"cluster {k} ({len(c)} points): residual rms {rms!r} in the band")
    return bad


# ------------------------------------------------------------------------- direct fit clusters

def random_arc(rng, sigma):
    """One arc of the direct fit tests: n ∈ [4, 40) points, centre uniform in ±2 m, r ∈ [0.02, 0.3],
    span ∈ [0.5, 3.0] rad, Gaussian point noise σ."""
    n = int(rng.integers(4, 40))
    c = rng.uniform(-2, 2, 2)
    r = rng.uniform(0.02, 0.3)
    t0 = rng.uniform(-math.pi, math.pi)
    t = t0 + np.sort(rng.uniform(0, rng.uniform(0.5, 3.0), n))
    pts = np.stack([c[0] + r * np.cos(t), c[1] + r * np.sin(t)], 1)
    if sigma > 0.0:
        pts = pts + rng.normal(0.0, sigma, pts.shape)
    return pts


def fit_arcs(sigma, count, seed):
    """(``count`` seeded arcs at noise σ with those inside the ill-determined band dropped,
    the number dropped)."""
    rng = np.random.default_rng([seed, FIT_SIGMAS.index(sigma)])
    arcs = [random_arc(rng, sigma) for _ in range(count)]
    kept = [a for a in arcs if not in_band(a)]
    return kept, count - len(kept)


def triples(count, seed):
    """Three points of a circle each, r ∈ [0.02, 0.3], at least 0.4 rad apart: (clusters, the
    circles [count, 3] they were drawn from)."""
    rng = np.random.default_rng(seed)
    cl, want = [], []
    for _ in range(count):
        c = rng.uniform(-2, 2, 2)
        r = rng.uniform(0.02, 0.3)
        t = rng.uniform(-math.pi, math.pi) + np.cumsum(rng.uniform(0.4, 1.5, 3))
        cl.append(np.stack([c[0] + r * np.cos(t), c[1] + r * np.sin(t)], 1))
        want.append((c[0], c[1], r))
    return cl, np.array(want)


def circumcircle(p):
    """Closed-form circle through three points, computed about the first one."""
    (ax, ay), (bx, by), (cx, cy) = p
    bx, by, cx, cy = bx - ax, by - ay, cx - ax, cy - ay
    d = 2.0 * (bx * cy - by * cx)
    ux = (cy * (bx * bx + by * by) - by * (cx * cx + cy * cy)) / d
    uy = (bx * (cx * cx + cy * cy) - cx * (bx * bx + by * by)) / d
    return ax + ux, ay + uy, math.hypot(ux, uy)
