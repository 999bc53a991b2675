"""Dev tool: the lidar Monte-Carlo run (ekf_sim_run_lidar), its laser kernel against lm_simulate's.

Shape: F = 64 filters, T = 20 messages per run, 360 beams, range_max = 3.5 m, on synth.swarm maps of
L cylinders (±max(0.5·√L, 2) m: at L = 1024 most of a map is beyond the laser's reach, at L = 20
none of it is). By default L = 20 and L = 1024.

  swarm   k_lidar_scan_swarm inside Sim.run_lidar as shipped: poses and maps read where the
          simulator keeps them, the scene culled to range_max while it is staged when the map has
          at least kCullFromMap cylinders (lm_launch.hpp) and staged whole below that.
  plain   k_lidar_scan through Detector.simulate(ranges=False) on the same T·F poses (the run's
          recorded truth) and the same F scenes (scene s = s mod F): each beam tests each cylinder.
  --forms adds the swarm kernel forced to cull (EKF_LIDAR_CULL_FROM=0) and forced not to
          (EKF_LIDAR_CULL_FROM above every map), the sweep kCullFromMap is read from.

All kernel times are HIP events around the dispatch (lm_last_simulate_us). The forms are taken in
turn, round after round, the order rotating by one each round (--reps of each after --warmup
untimed rounds; every run drives the robots further round the circle, so the poses move but the
shape does not; k_lidar_scan takes the poses of the run before it), and reported as median with
min / max. The first kernel of a round follows the host's own work between rounds and pays for a
GPU that has been idle: those samples are also reported on their own. run_lidar's wall time per
message is a host clock around the shipped form's call and the filter's sync. That the kernels
write the same bits is tests/test_gpu_sim_lidar.py's business, not this tool's; it still compares
them noiseless on the first run and says so.

Prints one JSON line per L.

  python tools/lidar_mc_bench.py [--reps 20] [--warmup 2] [--maps 20 1024] [--forms]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ekf-slam_amd"))
import pyekf  # noqa: E402
from pyekf import synth  # noqa: E402
from pyekf.landmarks import Detector  # noqa: E402

F, T, B = 64, 20, 360
LID = dict(n_beams=B, max_markers=32, obstacle_radius=0.038, seed=777, arena=(60.0, 60.0),
           range_max=3.5, sigma=1e-3)
KNOB = "EKF_LIDAR_CULL_FROM"
FORMS = {"swarm": None, "swarm_culled": "0", "swarm_whole": "1000000"}


def spread(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v), "reps": len(v)}


def knob(value):
    if value is None:
        os.environ.pop(KNOB, None)
    else:
        os.environ[KNOB] = value


def run(L, a):
    N = max(L, 50)
    sw = synth.swarm(N, F, T, survey=False, n_map=L)
    tpm = sw.wheel.shape[1]
    sim_kw = dict(seed=int(sw.seeds[0]), ticks_per_msg=tpm, max_markers=min(16, L),
                  marker_stride=16, start_theta=sw.start_pose[0], start_x=sw.start_pose[1],
                  start_y=sw.start_pose[2], record=1)
    e = pyekf.EKF(n_landmarks=N, n_filters=F)
    sim = pyekf.Sim(e, sw.landmarks, **sim_kw)
    det, plain = Detector(max_scans=T * F, max_beams=B), Detector(max_scans=T * F, max_beams=B)
    scenes = np.concatenate([sw.landmarks, np.full((F, L, 1), LID["obstacle_radius"])], 2)
    scene = (np.arange(T * F) % F).astype(np.int32)
    kw = dict(n_beams=B, arena=LID["arena"], range_max=LID["range_max"])
    forms = list(FORMS) if a.forms else ["swarm"]
    slots = forms + ["plain"]
    us = {k: [] for k in slots}
    first_us = {k: [] for k in slots}  # the same, when the form was the first of its round
    wall_ms = []
    same = {}
    poses = np.ascontiguousarray(sw.truth[:T], dtype=np.float64).reshape(T * F, 3)
    for rep in range(a.warmup + a.reps):
        k0 = rep % len(slots)
        for pos, form in enumerate(slots[k0:] + slots[:k0]):
            if form == "plain":
                plain.simulate(poses, scenes, scene, ranges=False, sigma=LID["sigma"], **kw)
                t_us = plain.last_simulate_us()
            else:
                knob(FORMS[form])
                t0 = time.perf_counter()
                sim.run_lidar(det, sw.cmd, **LID)
                e.sync()
                wall = time.perf_counter() - t0
                t_us = det.last_simulate_us()
                poses = sim.poses()[1].reshape(T * F, 3)
                if form == "swarm" and rep >= a.warmup:
                    wall_ms.append(1e3 * wall)
            if rep >= a.warmup:
                us[form].append(t_us)
                if pos == 0:
                    first_us[form].append(t_us)
        if rep == 0:  # noiseless bits (the noise is seeded per filter in one, not in the other)
            e2, d2 = pyekf.EKF(n_landmarks=N, n_filters=F), Detector(max_scans=T * F, max_beams=B)
            for form in forms:
                knob(FORMS[form])
                s2 = pyekf.Sim(e2, sw.landmarks, **sim_kw)
                s2.run_lidar(d2, sw.cmd, **dict(LID, sigma=0.0))
                got = d2.fetch_ranges()
                want = plain.simulate(s2.poses()[1].reshape(T * F, 3), scenes, scene, sigma=0.0,
                                      **kw)
                same[form] = bool(got.tobytes() == want.tobytes())
                s2.close()
            e2.close()
            d2.close()
    knob(None)
    cnt, _ = det.fetch_markers()
    out = {"L": L, "N": N, "filters": F, "messages": T, "beams": B, "range_max": LID["range_max"],
           "path": "resident" if e.path == pyekf.EKF_PATH_RESIDENT else "pipeline",
           "kernel_us": {k: spread(v) for k, v in us.items()},
           "kernel_us_first_in_round": {k: spread(v) for k, v in first_us.items() if v},
           "over_plain": {k: statistics.median(us[k]) / statistics.median(us["plain"])
                          for k in forms},
           "run_lidar_wall_ms": spread(wall_ms),
           "run_lidar_wall_ms_per_message": statistics.median(wall_ms) / T,
           "scans_with_markers": int((cnt > 0).sum()), "scans": T * F,
           "noiseless_bits_equal": same}
    for h in (sim, e, det, plain):
        h.close()
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--maps", type=int, nargs="+", default=[20, 1024])
    ap.add_argument("--forms", action="store_true")
    a = ap.parse_args()
    for L in a.maps:
        run(L, a)


if __name__ == "__main__":
    main()
