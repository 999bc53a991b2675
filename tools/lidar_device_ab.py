#!/usr/bin/env python3
"""Scans → final pose with and without the host hop between the landmark front-end and the filter.

F robots × T simulated scans (lm_simulate: 360 beams, 20 cylinders in a 5 m × 4 m arena, each
robot on the unit circle at its own phase), N landmark slots, fp64. Two ways from the scans
resident on the GPU to the posterior, alternated in one process after a warm-up of both:

  host hop   lm_detect_resident (markers and counts to the host, synchronising) → repack →
             ekf_replay(assoc = 1) (range / bearing and the plan on the host, one upload) → ekf_sync
  in place   lm_detect_device → lm_replay_into (k_plan_assoc plans from the marker buffer) → ekf_sync

Every repetition starts from ekf_reset, outside the timed region. Prints one line per repetition,
both medians, the corrections applied per repetition and the largest final-pose difference between
the two ways; --out also writes that as JSON.

  python tools/lidar_device_ab.py [--filters 8] [--scans 100] [--landmarks 256] [--max-markers 32]
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

import pyekf  # noqa: E402
from pyekf import synth  # noqa: E402
from pyekf.landmarks import Detector  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--filters", type=int, default=8)
    ap.add_argument("--scans", type=int, default=100)
    ap.add_argument("--landmarks", type=int, default=256)
    ap.add_argument("--max-markers", type=int, default=32)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    F, T, M = a.filters, a.scans, a.max_markers
    _, obs, _ = synth.lidar_world(n_scans=2)
    ang = 0.05 * np.arange(T)[:, None] + 2 * math.pi * np.arange(F)[None, :] / F
    poses = np.stack([ang + math.pi / 2, np.cos(ang), np.sin(ang)], 2)  # [T, F, 3], scan t·F + f
    det = Detector(max_scans=T * F, max_beams=360)
    det.simulate(poses.reshape(T * F, 3), obs, ranges=False, arena=(5.0, 4.0), sigma=1e-3)
    ekf = pyekf.EKF(n_landmarks=a.landmarks, n_filters=F)
    assert ekf.path == pyekf.EKF_PATH_PIPELINE and ekf.assoc_route != pyekf.EKF_ASSOC_MARKER

    def host_hop():
        cnt, mk = det.detect_resident(max_markers=M)
        c = np.clip(cnt, 0, M).astype(np.int32).reshape(T, F)
        rel = np.empty((T, F, M, 2))
        rel[..., 0] = mk["x"].reshape(T, F, M)
        rel[..., 1] = mk["y"].reshape(T, F, M)
        ekf.replay(c, rel, poses, assoc=True)
        ekf.sync()
        return int(c.sum())

    def in_place():
        det.detect_device(max_markers=M)
        rc = det.replay_into(ekf, T, poses)
        if rc != pyekf.EKF_OK:
            raise pyekf.EkfError(rc, "lm_replay_into")
        ekf.sync()
        return None

    ways = (("host_hop", host_hop), ("in_place", in_place))
    times = {name: [] for name, _ in ways}
    final, corrections = {}, 0
    for rep in range(-1, a.reps):  # rep −1: warm-up of both ways
        for name, fn in ways:
            ekf.reset()
            t0 = time.perf_counter()
            n = fn()
            dt = time.perf_counter() - t0
            corrections = n if n is not None else corrections
            final[name] = np.stack([ekf.pose(f) for f in range(F)])
            flags = [ekf.status(f) for f in range(F)]
            if rep >= 0:
                times[name].append(dt)
                print(f"rep {rep} {name:9s} {1e3 * dt:8.3f} ms  status {sorted(set(flags))}")
    res = {"filters": F, "scans": T, "landmarks": a.landmarks, "max_markers": M,
           "chunk_launches_per_scan": (M + 15) // 16, "corrections": corrections,
           "host_hop_ms": [1e3 * t for t in times["host_hop"]],
           "in_place_ms": [1e3 * t for t in times["in_place"]],
           "host_hop_median_ms": 1e3 * statistics.median(times["host_hop"]),
           "in_place_median_ms": 1e3 * statistics.median(times["in_place"]),
           "final_pose_max_diff": float(np.abs(final["host_hop"] - final["in_place"]).max())}
    print(f"medians: host hop {res['host_hop_median_ms']:.3f} ms, in place "
          f"{res['in_place_median_ms']:.3f} ms; {corrections} corrections per repetition; "
          f"final poses differ by at most {res['final_pose_max_diff']:.3e}")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(res, fh, indent=1)
    det.close()
    ekf.close()


if __name__ == "__main__":
    main()
