"""Named inputs for the simulator's obstacle collisions (ekf_sim_set_collisions, include/ekf_sim.h;
collide_wheels in ekf-slam_amd/csrc/sim_kernels.hip), in the style of tests/sim_cases.py: every case
is built from pyekf.synth alone (no GPU) and holds the host restatement (``synth.Swarm``, whose
``hits`` are the colliding ticks per message), the ``pyekf.Sim`` keywords that reproduce it on the
device, the radii and the run boundaries. tests/test_sim_collide_cases.py pins on the CPU that each
case reaches the path it is named for; tests/test_gpu_sim_collide.py runs them on the device.

The rule (nusim.cpp:232-254): once per tick, after FKin, the landmarks are tested in id order and the
pose is pushed out of the first one with d < R, R = collision_radius + obstacle_radius.

The robot drives straight along +x from the origin at 0.5 m/s and 200 Hz (2.5 mm a tick) unless a
case says otherwise; with slip 0 and equal wheel commands every tick is a pure translation, so the
tick at which a contact begins is set by the geometry alone:
  head-on        one cylinder on the x axis: the robot is held at cx − R while odometry goes on
  glance         a cylinder 0.1 m off the axis: the robot slides round it (> 40 ticks) and leaves
  first-tick     the first contact falls on tick 0 of message 2
  last-tick      the first contact falls on the last tick of message 1
  over-message   a glancing contact that begins in one message and ends in a later one (slip on)
  run-split      head-on, the drive cut into two runs inside the contact
  ticks-1/-64    1 and 64 ticks per message
  map-1/-65/-1024  map sizes: in the larger two a pair of overlapping cylinders lies on the path,
                 the lower id in another lane and another block of 64 than the higher (3 and 64;
                 700 and 1023). The higher id is nearer, so it is hit first, alone; from the tick
                 at which the pose is inside both the lower one acts
  start-inside   the start pose is inside a cylinder: tick 0 pushes it by nearly R
  chain          eight overlapping cylinders 0.05 m apart along y, ids rising with y: each tick the
                 robot is pushed out of one into the next, 0.05 m a tick against ρ = 0.02 m a
                 message, far out of reach of the candidate list built at the message's start
  one-of-two     two filters with maps of their own, only filter 0's has a cylinder on the path
  clear          collisions on, nothing within reach (a case of tests/sim_cases.py)

Decidability (``guard``): device and host poses agree to 1e-9 (SIM_TOL), so no test d < R that the
host restatement ran may have |d − R| < GAP = 1e-6 (``Swarm.hit_edge``), and the markers obey
sim_cases.guard as every simulator case does. A case that fails gets another seed or geometry, never
a looser comparison. (A tick after a push the pose is at d = R from that cylinder to rounding; the
next test of it comes a 2.5 mm tick later, which leaves |d − R| ≥ s²/2R = 2.1e-5 even for a step
along the tangent. That is why no case here drives slower.)
"""
from __future__ import annotations

import math
from dataclasses import dataclass

import numpy as np

import sim_cases as sc
from pyekf import synth

GAP = sc.GAP
COLLISION_RADIUS = 0.11      # diff_params.yaml: collision_radius
OBSTACLE_RADIUS = 0.038      # basic_world.yaml: obstacles.r
R = COLLISION_RADIUS + OBSTACLE_RADIUS
HZ, V = 200.0, 0.5
STEP = V / HZ                # m per tick
FAR = 40.0                   # where a map's unused landmarks are parked (beyond max_range)


@dataclass
class Case(sc.Case):
    collision_radius: float = COLLISION_RADIUS
    obstacle_radius: float = OBSTACLE_RADIUS
    start: tuple = (0.0, 0.0, 0.0)

    @property
    def hits(self) -> np.ndarray:
        """[T, F] colliding ticks per message of the host restatement."""
        return self.sw.hits


def straight(T, tpm=40, v=V, hz=HZ) -> synth.Drive:
    nt = T * tpm
    return synth.Drive(np.full(nt, v), np.zeros(nt), np.zeros(T, np.int32), tpm, hz)


def _make(name, landmarks, T, *, N=None, tpm=40, slip=0.0, seed=1200, bounds=None,
          start=(0.0, 0.0, 0.0), collision_radius=COLLISION_RADIUS, drive=None, max_range=5.0,
          n_filters=None) -> Case:
    lm = np.asarray(landmarks, np.float64)
    lm = lm[None] if lm.ndim == 2 else lm
    F = lm.shape[0] if n_filters is None else n_filters
    lm = np.broadcast_to(lm, (F,) + lm.shape[1:]).copy()
    L = lm.shape[1]
    N = max(L, 2) if N is None else N
    if drive is None:
        drive = straight(T, tpm)
    seeds = np.uint64(seed) + np.arange(F, dtype=np.uint64)
    sw = synth._generate(N, drive, seeds, lm, max_markers=16, start_pose=start, sensor_sigma=1e-3,
                         slip=slip, max_range=max_range, collision_radius=collision_radius,
                         obstacle_radius=OBSTACLE_RADIUS)
    kw = dict(seed=int(seed), f0=0, ticks_per_msg=int(tpm), slip=float(slip), sensor_sigma=1e-3,
              max_range=float(max_range), max_markers=16, marker_stride=int(sw.ids.shape[2]),
              start_theta=float(start[0]), start_x=float(start[1]), start_y=float(start[2]),
              record=1)
    return Case(name, sw, kw, tuple(bounds) if bounds else ((0, T),), N, float(max_range), 16,
                False, collision_radius, OBSTACLE_RADIUS, tuple(start))


def contact_x(first_tick):
    """The centre of a cylinder on the x axis that a straight drive from the origin first touches
    at (0-based) tick ``first_tick``: half a step inside then, half a step outside a tick before."""
    return R + STEP * (first_tick + 1) - 0.5 * STEP


def pair_map(L, low, high, seed):
    """L landmarks: ``high`` at (0.5, 0.08) and ``low`` at (0.5049, −0.12) overlap ahead of the
    path (the straight drive reaches ``high`` first, slides down its side and is inside both some
    twenty ticks later); the others are random ones, any within 1 m of the path's segment parked FAR
    away."""
    lm = synth.random_landmarks(L, seed)
    near = (lm[:, 0] > -1.0) & (lm[:, 0] < 2.0) & (np.abs(lm[:, 1]) < 1.0)
    lm[near, 1] += FAR
    lm[high] = (0.5, 0.08)
    lm[low] = (0.5049, -0.12)
    return lm


def chain_map(L=40, links=8):
    """``links`` cylinders at (0, −0.1 + 0.05·i), i = id: the first holds the start pose (0, 0); the
    other landmarks are parked FAR away."""
    lm = np.zeros((L, 2))
    lm[:, 0] = FAR + np.arange(L)
    lm[:links, 0] = 0.0
    lm[:links, 1] = -0.1 + 0.05 * np.arange(links)
    return lm


def _clear() -> Case:
    """sim_cases' size-64 (random_landmarks keeps 0.3 m off the circle) with collisions on."""
    base = sc.get("size-64")
    sw = base.sw
    drive = synth.circle_drive(sw.count.shape[0], 1.0, 0.5, 200.0, 40)
    sw2 = synth._generate(base.n_slots, drive, sw.seeds, sw.landmarks, max_markers=16,
                          start_pose=sw.start_pose, sensor_sigma=1e-3, slip=0.02, max_range=5.0,
                          collision_radius=COLLISION_RADIUS, obstacle_radius=OBSTACLE_RADIUS)
    return Case("clear", sw2, dict(base.sim_kw), base.bounds, base.n_slots, base.max_range, base.m,
                False, COLLISION_RADIUS, OBSTACLE_RADIUS, tuple(sw.start_pose))


_BUILDERS = {
    "head-on": lambda: _make("head-on", [[0.5013, 0.0]], 8),
    "glance": lambda: _make("glance", [[0.5, 0.1]], 8),
    "first-tick": lambda: _make("first-tick", [[contact_x(2 * 40), 0.0]], 5),
    "last-tick": lambda: _make("last-tick", [[contact_x(2 * 40 - 1), 0.0]], 5),
    "over-message": lambda: _make("over-message", [[0.5, 0.1], [3.0, 2.0]], 8, slip=0.02,
                                  seed=1210),
    "run-split": lambda: _make("run-split", [[0.5013, 0.0]], 8, bounds=((0, 5), (5, 8))),
    "ticks-1": lambda: _make("ticks-1", [[R + 2.5 * STEP, 0.0]], 8, tpm=1),
    "ticks-64": lambda: _make("ticks-64", [[0.5, 0.1], [3.0, 2.0]], 5, tpm=64, slip=0.02,
                              seed=1220),
    "map-1": lambda: _make("map-1", [[0.5013, 0.0]], 6, slip=0.02, seed=1230),
    "map-65": lambda: _make("map-65", pair_map(65, 3, 64, 1265), 6),
    "map-1024": lambda: _make("map-1024", pair_map(1024, 700, 1023, 2024), 6),
    "start-inside": lambda: _make("start-inside", [[0.05, 0.02], [3.0, 2.0]], 4),
    "chain": lambda: _make("chain", chain_map(), 6, tpm=8),
    "one-of-two": lambda: _make("one-of-two", [[[0.5013, 0.0], [3.0, 2.0]],
                                               [[0.5013, 1.0], [3.0, 2.0]]], 8, slip=0.02,
                                seed=1240),
    "clear": _clear,
}
NAMES = tuple(_BUILDERS)
_cache: dict = {}


def get(name) -> Case:
    if name not in _cache:
        _cache[name] = _BUILDERS[name]()
    return _cache[name]


def simulate(case):
    """The host restatement again, tick by tick: (truth [F, T, 3], path [F, ticks, 2], hits [F, T],
    edge) of synth._simulate with the case's collisions."""
    sw = case.sw
    T, tpm = sw.count.shape[0], sw.wheel.shape[1]
    drive = drive_of(case)
    assert drive.v.shape[0] == T * tpm
    _, truth, path, hits, edge = synth._simulate(
        drive, sw.seeds, sw.start_pose, case.sim_kw["slip"], sw.landmarks,
        case.collision_radius, case.obstacle_radius)
    return truth, path, hits, edge


def drive_of(case) -> synth.Drive:
    T, tpm = case.sw.count.shape[0], case.sw.wheel.shape[1]
    return synth.circle_drive(T, 1.0, 0.5, 200.0, 40) if case.name == "clear" else straight(T, tpm)


def rho(case) -> np.ndarray:
    """[T, F] the candidate list's ρ of every message as the kernel's header comment defines it:
    (Σ_j |radius/2·(dl_j + dr_j)|)·(1 + 2⁻²⁰) over the message's slipped wheel increments."""
    sw = case.sw
    T, tpm = sw.count.shape[0], sw.wheel.shape[1]
    k = np.arange(T * tpm, dtype=np.uint64)
    u = synth.rng_uniform(sw.seeds[:, None, None], synth._S_SLIP,
                          k[None, :, None] * np.uint64(2) + np.arange(2, dtype=np.uint64))
    slipped = sw.cmd[None] * (1.0 + case.sim_kw["slip"] * (2.0 * u - 1.0))       # [F, nt, 2]
    vx = np.abs(synth.WHEEL_RADIUS / 2.0 * (slipped[..., 0] + slipped[..., 1]))
    return vx.reshape(len(sw.seeds), T, tpm).sum(2).T * (1.0 + 2.0 ** -20)


def guard(case) -> float:
    """The decidability guard of the module docstring: raises where it fails, returns the smallest
    |d − R| over the host restatement's tests."""
    assert case.sw.hit_edge > GAP, (case.name, case.sw.hit_edge)
    assert sc.guard(case) > GAP
    return float(case.sw.hit_edge)
