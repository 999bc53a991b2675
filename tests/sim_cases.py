"""Named inputs for the on-device simulator (ekf-slam_amd/csrc/sim_kernels.hip) off the one point
of its parameter space that the rest of the suite runs it at: map sizes around the 64-lane wave and
the 1024 limit, 1 to 64 ticks per message, 1 and 15 markers, ties in the selection, messages with no
marker, every ordering of the three sensing modes, the survey's out-of-range fallback, a marker
stride wider than the marker count, a non-zero f0, no noise, and runs of growing length.

Every case is built from pyekf.synth alone (no GPU): a ``Case`` holds the host restatement
(``synth.Swarm``), the ``pyekf.Sim`` keyword arguments that reproduce it on the device, and the run
boundaries. tests/test_sim_cases.py pins on the CPU that each case reaches the path it is named
for and that it is decidable; tests/test_gpu_sim_edges.py runs them on the device.

Decidability (``guard``): device and host true poses agree to 1e-9 (SIM_TOL of
tests/test_gpu_sim.py), so distances agree to a few 1e-8 over these fields, while ids and counts
are compared exactly. The reference must therefore not lie within rounding of a different answer:
with GAP = 1e-6 (about 50 times that disagreement), any two distances that compete for a place
must be bit-equal (the duplicated coordinates of ``ties``) or more than GAP apart, and none may lie
within GAP of the message's effective range (max_range, 2·max_range for SURVEY). A case that fails
the guard gets another seed, never a looser comparison.

``select`` restates the selection landmark by landmark (ids only), under the simulator's sighted
rule ("survey": a landmark is sighted once a SURVEY message has reported it; NEAREST and ALL
messages neither read nor write the set) or under the rule the host restatement had before
("any": every reported landmark is sighted, DELETE markers of ALL included). The two differ once a
NEAREST or ALL message precedes a SURVEY one (``nearest-then-survey``).
"""
from __future__ import annotations

import math
from dataclasses import dataclass

import numpy as np

from pyekf import synth

GAP = 1e-6
NEAREST, SURVEY, ALL = synth.SENSE_NEAREST, synth.SENSE_SURVEY, synth.SENSE_ALL


@dataclass
class Case:
    name: str
    sw: synth.Swarm
    sim_kw: dict            # pyekf.Sim(e, sw.landmarks, **sim_kw) reproduces sw on the device
    bounds: tuple           # the runs, ((first message, one past the last), ...)
    n_slots: int            # the filter's landmark slots N
    max_range: float
    m: int                  # max_markers as configured (the device clamps it to the map size)
    basic_world: bool = False  # 4 landmarks, every one always reported (the oracle's 1e-8 bounds)

    @property
    def stride(self) -> int:
        return int(self.sw.ids.shape[2])

    @property
    def n_map(self) -> int:
        return int(self.sw.landmarks.shape[1])

    @property
    def nearest_only(self) -> bool:
        return not (self.sw.sense != NEAREST).any()

    @property
    def parallel(self) -> bool:
        """Whether a pipeline handle may run the case in the parallel form (sim_api.cpp
        parallel_ok: no SURVEY message, a stride within one chunk)."""
        return not (self.sw.sense == SURVEY).any() and self.stride <= 16


def _maps(L, seed, F):
    return np.stack([synth.random_landmarks(L, seed + f) for f in range(F)])


def _make(name, L, N, F, T, *, map_seed=None, seed=900, tpm=40, sense=NEAREST, m=16, max_range=5.0,
          f0=0, slip=0.02, sigma=1e-3, marker_stride=None, landmarks=None, bounds=None,
          drive=None, start_pose=(0.0, 0.0, -1.0), basic_world=False) -> Case:
    if drive is None:
        drive = synth.circle_drive(T, 1.0, 0.5, 200.0, tpm)
    drive.sense = np.broadcast_to(np.asarray(sense, np.int32), (T,)).copy()
    if landmarks is None:
        landmarks = _maps(L, map_seed, F)
    seeds = np.uint64(seed) + np.uint64(f0) + np.arange(F, dtype=np.uint64)
    sw = synth._generate(N, drive, seeds, landmarks, max_markers=m, start_pose=start_pose,
                         sensor_sigma=sigma, slip=slip, max_range=max_range,
                         marker_stride=marker_stride)
    kw = dict(seed=int(seed), f0=int(f0), ticks_per_msg=int(tpm), slip=float(slip),
              sensor_sigma=float(sigma), max_range=float(max_range), max_markers=int(m),
              marker_stride=int(sw.ids.shape[2]), start_theta=float(sw.start_pose[0]),
              start_x=float(sw.start_pose[1]), start_y=float(sw.start_pose[2]), record=1)
    return Case(name, sw, kw, tuple(bounds) if bounds else ((0, T),), N, float(max_range), int(m),
                basic_world)


# ---- the cases -----------------------------------------------------------------------------------
SIZES = (1, 2, 63, 64, 65, 1023, 1024)
TICKS = (1, 2, 63, 64)


def _size(L, name=None, **kw):
    """NEAREST, 16 markers, L landmarks in N = max(L, 2) slots (N = 1024 for L = 1023: L < N)."""
    N = 1024 if L == 1023 else max(L, 2)
    kw.setdefault("T", 6)
    return _make(name or f"size-{L}", L, N, 2, map_seed=3000 + L, seed=900, **kw)


def _ticks(tpm, L=64, name=None):
    return _make(name or f"ticks-{tpm}", L, L, 2, 5, map_seed=3100 + tpm, seed=910, tpm=tpm)


def _markers(m, map_seed, L=64, name=None):
    return _make(name or f"markers-{m}", L, L, 2, 6, map_seed=map_seed, seed=920, m=m)


def ties_map(first=7) -> np.ndarray:
    """130 landmarks: 64 points on a circle of radius 2.5 about the origin, each one again 64 ids
    later (the same lane of the sensing wave, its next slot), and two more copies in other lanes
    (ids 128, 129 = points first, first + 1: lanes 0 and 1). The drive stays near point 48, so
    points 7, 8 are never in range; ``ties-cross`` copies points 48, 49 instead, whose three-way
    ties then span two lanes."""
    a = 2.0 * math.pi * np.arange(64) / 64.0
    base = 2.5 * np.stack([np.cos(a), np.sin(a)], 1)
    lm = np.zeros((130, 2))
    lm[:64] = base
    lm[64:128] = base
    lm[128:130] = base[first:first + 2]
    return lm


def _ties(m, first=7, name=None):
    return _make(name or f"ties-{m}", 130, 130, 1, 6, seed=930, m=m, max_range=2.0,
                 landmarks=ties_map(first)[None])


def _basic_world_all(name, F, T, seed, max_range, bounds=None):
    drive = synth.circle_drive(T, 0.3, 0.5, 200.0, 40)
    return _make(name, 4, 50, F, T, seed=seed, sense=ALL, max_range=max_range, drive=drive,
                 landmarks=np.broadcast_to(synth.BASIC_WORLD_LANDMARKS, (F, 4, 2)),
                 start_pose=(synth.BASIC_WORLD_THETA0, 0.0, 0.0), basic_world=True, bounds=bounds)


_BUILDERS = {
    **{f"size-{L}": (lambda L=L: _size(L)) for L in SIZES},
    **{f"ticks-{t}": (lambda t=t: _ticks(t)) for t in TICKS},
    "markers-1": lambda: _markers(1, 3204),   # (3201 fails the guard: two distances 3e-7 apart)
    "markers-15": lambda: _markers(15, 3215),
    "ties-16": lambda: _ties(16),
    "ties-15": lambda: _ties(15),
    "ties-cross": lambda: _ties(16, 48, "ties-cross"),
    # messages with no marker: in the middle, at the end of a run, at the start of the next
    "empty": lambda: _make("empty", 12, 40, 3, 12, map_seed=4400, seed=50, max_range=0.8,
                           bounds=((0, 5), (5, 12))),
    "empty-tail": lambda: _make("empty-tail", 20, 40, 3, 12, map_seed=4402, seed=50,
                                max_range=0.8),
    "nearest-then-survey": lambda: _make("nearest-then-survey", 40, 64, 2, 8, map_seed=5, seed=5,
                                         m=4, max_range=2.5, sense=[0, 0, 0, 1, 1, 1, 0, 1]),
    "mixed-all": lambda: _make("mixed-all", 12, 20, 2, 10, map_seed=4200, seed=60, m=3,
                               marker_stride=12, max_range=1.6,
                               sense=[0, 1, 2, 1, 0, 1, 1, 2, 0, 1]),
    # the basic world from 0.86 m and more away: the first six messages are DELETE throughout, so
    # both runs begin with chunks of no correction and the first ends with one
    "all-delete": lambda: _basic_world_all("all-delete", 2, 12, 70, 0.75, ((0, 4), (4, 12))),
    "survey-fallback": lambda: _make("survey-fallback", 40, 64, 2, 4, map_seed=4412, seed=80, m=4,
                                     max_range=0.5, sense=SURVEY),
    "stride-20": lambda: _size(64, "stride-20", marker_stride=20),
    "stride-65": lambda: _size(64, "stride-65", marker_stride=65),
    "f0-seed": lambda: _make("f0-seed", 64, 64, 2, 6, map_seed=3064, seed=2 ** 63 + 12345, f0=3),
    "no-noise": lambda: _make("no-noise", 64, 64, 2, 6, map_seed=3064, seed=940, slip=0.0,
                              sigma=0.0),
    "growth": lambda: _size(64, "growth", T=14,
                            bounds=((0, 1), (1, 2), (2, 5), (5, 7), (7, 14))),
    # the resident path's N ≤ 62
    "ticks-64-small": lambda: _ticks(64, 40, "ticks-64-small"),
    "markers-1-small": lambda: _markers(1, 3201, 40, "markers-1-small"),
}
NAMES = tuple(_BUILDERS)
_cache: dict = {}


def get(name) -> Case:
    if name not in _cache:
        _cache[name] = _BUILDERS[name]()
    return _cache[name]


# ---- the case's own checks -----------------------------------------------------------------------
def distances(case) -> np.ndarray:
    """[T, F, L] true distance of every landmark at every message, from sw.truth and the map."""
    sw = case.sw
    dx = sw.landmarks[None, :, :, 0] - sw.truth[:, :, None, 1]
    dy = sw.landmarks[None, :, :, 1] - sw.truth[:, :, None, 2]
    return np.hypot(dx, dy)


def effective_range(case, t) -> float:
    return (synth.SURVEY_RANGE if case.sw.sense[t] == SURVEY else 1.0) * case.max_range


def guard(case) -> float:
    """The decidability guard of the module docstring for every message and filter: raises
    AssertionError where it fails, returns the worst (smallest) gap met."""
    d = distances(case)
    worst = math.inf
    for t in range(d.shape[0]):
        rng = effective_range(case, t)
        for f in range(d.shape[1]):
            v = np.sort(d[t, f])
            edge = float(np.abs(v - rng).min())
            assert edge > GAP, (case.name, t, f, "range", edge)
            worst = min(worst, edge)
            near = v[v <= rng + GAP]
            if near.size == 0:          # (the survey's fallback: the nearest, out of range)
                near = v[:2]
            step = np.diff(near)
            step = step[step != 0.0]    # bit-equal: the duplicated coordinates of the ties cases
            if step.size:
                assert step.min() > GAP, (case.name, t, f, "order", float(step.min()))
                worst = min(worst, float(step.min()))
    return worst


def select(case, rule="survey"):
    """The selected ids of every (message, filter), landmark by landmark: [T][F] lists. ``rule``:
    "survey" (the simulator's) or "any" (every reported landmark is sighted)."""
    assert rule in ("survey", "any")
    sw, d = case.sw, distances(case)
    T, F, L = d.shape
    m = min(case.m, L)
    sighted = [set() for _ in range(F)]
    out = []
    for t in range(T):
        mode, rng, row = int(sw.sense[t]), effective_range(case, t), []
        for f in range(F):
            if mode == ALL:
                ids = list(range(L))
            else:
                inr = [l for l in range(L) if d[t, f, l] <= rng]
                if mode == SURVEY:
                    if not inr:
                        inr = [int(np.argmin(d[t, f]))]
                    inr.sort(key=lambda l: (l in sighted[f], d[t, f, l], l))
                else:
                    inr.sort(key=lambda l: (d[t, f, l], l))
                ids = inr[:m]
            if mode == SURVEY or rule == "any":
                sighted[f].update(ids)
            row.append(ids)
        out.append(row)
    return out
