"""Dev tool: what the simulator's obstacle collisions (ekf_sim_set_collisions) cost.

Shape: F = 512 filters, T = 20 messages of 40 ticks per run, the unit circle of synth.swarm
(0.5 rad/s, 2.5 mm a tick, slip 0.02), maps of L landmarks uniform in ±max(0.5·√L, 2) m and none
within 0.4 m of the circle, on the HBM pipeline (EKF_RESIDENT=0), so ekf_sim_run takes the parallel
form: k_sim_arcs, k_sim_pose or k_sim_pose_collide, k_sim_sense. The simulators (one per form
below) share one fp32 filter handle and the commands, in three states:

  off       collisions off: the kernels of a simulator that never heard of them
  clear     collisions on, the same maps: nothing is ever in reach
  contact   collisions on, maps with eight landmarks moved onto the circle, 0.08 m off it to
            alternating sides and π/4 apart: the robot meets one every second message or so

and the collision kernel's candidate list in its three settings: as shipped (kCollideCullFromMap,
sim_launch.hpp), culled per message (EKF_SIM_CULL_FROM=1 when the simulator is created) and the
whole map staged once (EKF_SIM_CULL_FROM above every map). --sequential adds k_sim / k_sim_collide
(EKF_SIM_PARALLEL=0).

Times are HIP events around the simulator's launches of a run (EKF_SIM_TIMING, ekf_sim_last_us): the
wheel walk and the sensing, not the filter. The forms are taken in turn, round after round, the
order rotating by one each round (--reps of each after --warmup untimed rounds; every run drives the
robots further round the circle), and reported as median with min / max. Prints one JSON line per L.

  python tools/sim_collide_bench.py [--reps 40] [--warmup 2] [--maps 20 256 1024] [--sequential]
"""
import argparse
import json
import math
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ekf-slam_amd"))
os.environ["EKF_SIM_TIMING"] = "1"
os.environ["EKF_RESIDENT"] = "0"
import pyekf  # noqa: E402
from pyekf import synth  # noqa: E402

F, T, TPM = 512, 20, 40
COLLISION_RADIUS, OBSTACLE_RADIUS = 0.11, 0.038
KNOB = "EKF_SIM_CULL_FROM"
CULLS = {"shipped": None, "culled": "1", "whole": "1000000"}


def spread(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v), "reps": len(v)}


def env(name, value):
    if value is None:
        os.environ.pop(name, None)
    else:
        os.environ[name] = value


def maps(L, seed=11):
    """[F, L, 2] uniform in ±half, none within 0.4 m of the unit circle about the origin."""
    rng = np.random.default_rng(seed)
    half = max(0.5 * math.sqrt(L), 2.0)
    out = rng.uniform(-half, half, (F, L, 2))
    for _ in range(64):
        bad = np.abs(np.hypot(out[..., 0], out[..., 1]) - 1.0) < 0.4
        if not bad.any():
            break
        out[bad] = rng.uniform(-half, half, (int(bad.sum()), 2))
    assert not bad.any()
    return out


def in_the_way(lm, n=8):
    """The maps with their first n landmarks moved onto the circle."""
    out = lm.copy()
    for i in range(min(n, lm.shape[1])):
        ang, rad = i * 2.0 * math.pi / n + 0.3, 1.0 + (0.08 if i % 2 else -0.08)
        out[:, i] = (rad * math.sin(ang), -rad * math.cos(ang))
    return out


def run(L, a):
    N = max(L, 64)
    drive = synth.circle_drive(T, ticks_per_msg=TPM)
    dt = 1.0 / drive.tick_hz
    cmd = np.stack([(drive.v - drive.w * synth.TRACK_WIDTH / 2.0) / synth.WHEEL_RADIUS * dt,
                    (drive.v + drive.w * synth.TRACK_WIDTH / 2.0) / synth.WHEEL_RADIUS * dt], 1)
    lm = maps(L)
    e = pyekf.EKF(n_landmarks=N, n_filters=F, dtype=pyekf.EKF_F32)
    assert e.path == pyekf.EKF_PATH_PIPELINE
    kw = dict(seed=20240317, ticks_per_msg=TPM, max_markers=min(16, L), marker_stride=16,
              start_theta=0.0, start_x=0.0, start_y=-1.0, record=0)
    forms = [("off", "shipped", "1")] + [(s, c, "1") for s in ("clear", "contact") for c in CULLS]
    if a.sequential:
        forms += [(s, "shipped", "0") for s in ("off", "clear", "contact")]
    # a simulator per form (the list's setting is read when a simulator is created), one handle
    sims = {}
    for form in forms:
        state, cull, _ = form
        env(KNOB, CULLS[cull])
        sims[form] = pyekf.Sim(e, in_the_way(lm) if state == "contact" else lm, **kw)
        if state != "off":
            sims[form].set_collisions(COLLISION_RADIUS, OBSTACLE_RADIUS)
    env(KNOB, None)
    us = {f: [] for f in forms}
    for rep in range(a.warmup + a.reps):
        k0 = rep % len(forms)
        for form in forms[k0:] + forms[:k0]:
            env("EKF_SIM_PARALLEL", form[2])
            sims[form].run(cmd)
            t_us = sims[form].last_us()
            e.sync()
            if rep >= a.warmup:
                us[form].append(t_us)
    env("EKF_SIM_PARALLEL", None)
    states = ("off", "clear", "contact")
    hits = {s: sum(sims[f].collisions(per_msg=False)[0] for f in forms if f[0] == s)
            for s in states}
    runs = {s: sum(1 for f in forms if f[0] == s) * (a.warmup + a.reps) for s in states}
    name = lambda f: f"{f[0]}/{f[1]}" + ("" if f[2] == "1" else "/sequential")  # noqa: E731
    off = statistics.median(us[forms[0]])
    out = {"L": L, "N": N, "filters": F, "messages": T, "ticks_per_msg": TPM,
           "sim_us": {name(f): spread(v) for f, v in us.items()},
           "over_off": {name(f): statistics.median(v) / off for f, v in us.items()},
           "colliding_tick_fraction": {s: float(hits[s].sum()) / (runs[s] * T * TPM * F)
                                       for s in states},
           "filters_that_collided": {s: int((hits[s] > 0).sum()) for s in states}}
    for h in list(sims.values()) + [e]:
        h.close()
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--reps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--maps", type=int, nargs="+", default=[20, 256, 1024])
    ap.add_argument("--sequential", action="store_true")
    a = ap.parse_args()
    for L in a.maps:
        run(L, a)


if __name__ == "__main__":
    main()
