"""Dev tool: lidar scans made on the device and detected where they lie, against the host path.

Two shapes, the same poses and cylinders on both paths:
  surrogate  426 scans × 360 beams × 20 cylinders, one scene (synth.lidar_world: the rosbag shape)
  swarm      one message of a 4096-filter swarm: 4096 scans × 360 beams, each filter its own
             20 cylinders (4096 scenes)

  device  Detector.simulate(ranges=False) + Detector.detect_resident(): lm_simulate's kernel writes
          the range buffer the detection kernels read; up go poses and scenes, down come markers.
  host    synth.lidar_scans on the CPU (one call per scene: that is all it takes), then
          Detector.detect, which uploads the [S, 360] float32 ranges.

Prints one JSON line per shape: scans/s of both paths (median wall time of --reps calls, each ending
in the detection's stream synchronise, after --warmup untimed calls; the spread as min / max), the
host path's split into ray casting and detect, and the device time of the scan kernel
(lm_last_simulate_us) and of the detection kernels (lm_last_kernel_us) from HIP events. The two
paths draw their noise differently (numpy's generator against the counter RNG), so their scans are
two realisations of the same world, not the same bits; that the device's scans and detections are
right is tests/test_gpu_lidar_sim.py's business, not this tool's.

  python tools/lidar_sim_bench.py [--reps 200] [--host-reps 3] [--warmup 3] [--shape surrogate|swarm]
"""
import argparse
import json
import math
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ekf-slam_amd"))
from pyekf import synth  # noqa: E402
from pyekf.landmarks import Detector  # noqa: E402

INC = float(np.float32(2 * math.pi / 360))
ARENA = (5.0, 4.0)
SIGMA = 1e-3


def surrogate():
    sc, obs, _ = synth.lidar_world()
    return sc.truth, np.array(obs)[None], None


def swarm(F=4096, n_obstacles=20, seed=20240317):
    """Filter f stands somewhere on the unit circle, heading along it, among its own 20 cylinders of
    lidar_world's radius, none within 0.3 m of the robot."""
    rng = np.random.default_rng(seed)
    a = rng.uniform(0.0, 2.0 * math.pi, F)
    poses = np.stack([a + math.pi / 2, np.cos(a), np.sin(a)], 1)
    lo, hi = [-ARENA[0] / 2 + 0.5, -ARENA[1] / 2 + 0.5], [ARENA[0] / 2 - 0.5, ARENA[1] / 2 - 0.5]
    xy = rng.uniform(lo, hi, (F, n_obstacles, 2))
    while True:
        near = np.hypot(xy[..., 0] - poses[:, None, 1], xy[..., 1] - poses[:, None, 2]) < 0.3
        if not near.any():
            break
        xy[near] = rng.uniform(lo, hi, (int(near.sum()), 2))
    scenes = np.concatenate([xy, np.full((F, n_obstacles, 1), 0.038)], 2)
    return poses, scenes, np.arange(F, dtype=np.int32)


def timed(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return ts


def stats(ts, S):
    return {"scans_per_s": S / statistics.median(ts), "ms_median": 1e3 * statistics.median(ts),
            "ms_min": 1e3 * min(ts), "ms_max": 1e3 * max(ts), "reps": len(ts)}


def run(name, poses, scenes, scene, a):
    S = len(poses)
    det = Detector(max_scans=S, max_beams=360)

    def device():
        det.simulate(poses, scenes, scene, ranges=False, arena=ARENA, sigma=SIGMA, seed=1)
        return det.detect_resident()

    cast_s, detect_s = [], []

    def host():
        t0 = time.perf_counter()
        if scene is None:
            scans = synth.lidar_scans(poses, scenes[0], arena=ARENA, sigma=SIGMA, seed=1)
        else:
            scans = np.concatenate([synth.lidar_scans(poses[s], scenes[scene[s]], arena=ARENA,
                                                      sigma=SIGMA, seed=1 + s) for s in range(S)])
        t1 = time.perf_counter()
        cast_s.append(t1 - t0)
        out = det.detect(scans, np.zeros(S), np.full(S, INC))
        detect_s.append(time.perf_counter() - t1)
        return out

    dev = timed(device, a.reps, a.warmup)
    cd, _ = device()
    sim_us, det_us = det.last_simulate_us(), det.last_kernel_us()
    hst = timed(host, a.host_reps, 1)
    ch, _ = host()
    out = {"shape": name, "scans": S, "beams": 360, "cylinders": int(scenes.shape[1]),
           "scenes": int(scenes.shape[0]),
           "markers": {"device": int(cd[cd > 0].sum()), "host": int(ch[ch > 0].sum())},
           "device": stats(dev, S), "host": stats(hst, S),
           "host_raycast_ms_median": 1e3 * statistics.median(cast_s[1:]),
           "host_detect_ms_median": 1e3 * statistics.median(detect_s[1:]),
           "simulate_kernel_us": sim_us, "detect_kernels_us": det_us,
           "speedup": statistics.median(hst) / statistics.median(dev)}
    det.close()
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--host-reps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--shape", choices=["surrogate", "swarm"], action="append")
    a = ap.parse_args()
    for name in a.shape or ["surrogate", "swarm"]:
        run(name, *(surrogate() if name == "surrogate" else swarm()), a)


if __name__ == "__main__":
    main()
