"""Dev tool: what the pose trace (ekf_trace_*, include/ekf.h) costs when on, and what it buys.

  python tools/trace_ab.py [--reps 5] [--out trace_ab.json]

One process, alternating, medians over --reps repetitions after one warm-up of each leg:
  n1024_fp32   the headline replay (N = 1024 fp32 from an fp64 survey, ekf_replay_device, 20
               messages after 5) with the trace off and on;
  basic_world  the same on the resident path (N = 50 fp64, 20 messages after 5, one deferred
               submission);
  surrogate    the rosbag surrogate drive (426 scans, N = 50, unknown association) with both
               per-message outputs: slam_replay(out_pose, out_tmo), which synchronises per message,
               against slam_replay_trace, which reads them from the trace after one submission.
Prints one JSON object (times in µs, rates in corrections/s)."""
import argparse
import json
import math
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ekf-slam_amd"))

import pyekf  # noqa: E402
from pyekf import synth  # noqa: E402


def med(v):
    return float(np.median(v))


def headline(reps):
    import torch
    N, warm, pre, T = 1024, 40, 5, 20
    sc = synth.synthetic(N, warm + pre + T)
    odom = pyekf.odometry(sc)
    e64 = pyekf.EKF(n_landmarks=N)
    e64.replay(sc.count[:warm, None], sc.rel[:warm, None], odom[:warm, None],
               ids=sc.ids[:warm, None], actions=sc.actions[:warm, None])
    x0, S0, c0 = e64.state()
    tmo = e64.map_odom()
    e64.close()

    def gpu(sl):
        return [torch.from_numpy(np.ascontiguousarray(a[sl, None])).cuda() for a in
                (sc.count, sc.ids, sc.actions, sc.rel, odom)]
    gp, gt = gpu(slice(warm, warm + pre)), gpu(slice(warm + pre, warm + pre + T))
    M = sc.ids.shape[1]
    corr = int(sc.count[warm + pre:].sum())
    e = pyekf.EKF(n_landmarks=N, dtype=pyekf.EKF_F32)
    times = {False: [], True: []}
    for r in range(reps + 1):
        for on in (False, True):
            e.trace_enable(64 if on else 0)
            e.set_state(x0, S0, tmo=tmo, counter=c0)
            e.replay_device(gp[0], gp[3], gp[4], gp[1], gp[2])
            e.sync()
            t0 = time.perf_counter()
            e.replay_device_raw(T, M, gt[0].data_ptr(), gt[3].data_ptr(), gt[4].data_ptr(),
                                gt[1].data_ptr(), gt[2].data_ptr())
            e.sync()
            dt = time.perf_counter() - t0
            if on:
                assert e.trace_count() == pre + T
            if r:
                times[on].append(dt)
    e.close()
    return {"messages": T, "corrections": corr,
            "off_us_per_message": med(times[False]) / T * 1e6,
            "on_us_per_message": med(times[True]) / T * 1e6,
            "off_corrections_per_s": corr / med(times[False]),
            "on_corrections_per_s": corr / med(times[True]),
            "off_us_all": [t * 1e6 for t in times[False]],
            "on_us_all": [t * 1e6 for t in times[True]]}


def basic_world(reps):
    pre, T = 5, 20
    sc = synth.basic_world(pre + T)
    odom = pyekf.odometry(sc)
    e = pyekf.EKF(n_landmarks=50)
    assert e.path == pyekf.EKF_PATH_RESIDENT
    e.defer(True)
    corr = int(np.count_nonzero((np.arange(sc.ids.shape[1])[None] < sc.count[pre:, None]) &
                                (sc.actions[pre:] != synth.DELETE)))

    def feed(sl):
        e.replay(sc.count[sl, None], sc.rel[sl, None], odom[sl, None], ids=sc.ids[sl, None],
                 actions=sc.actions[sl, None])
    times = {False: [], True: []}
    for r in range(reps + 1):
        for on in (False, True):
            e.trace_enable(64 if on else 0)
            e.reset()
            feed(slice(0, pre))
            e.sync()
            t0 = time.perf_counter()
            feed(slice(pre, pre + T))
            e.sync()
            dt = time.perf_counter() - t0
            if on:
                assert e.trace_count() == pre + T
            if r:
                times[on].append(dt)
    e.close()
    return {"messages": T, "corrections": corr,
            "off_us_per_message": med(times[False]) / T * 1e6,
            "on_us_per_message": med(times[True]) / T * 1e6,
            "off_us_all": [t * 1e6 for t in times[False]],
            "on_us_all": [t * 1e6 for t in times[True]]}


def surrogate(reps):
    from pyekf.landmarks import Detector
    sc, _, scans = synth.lidar_world()
    T = len(scans)
    inc = float(np.float32(2 * math.pi / 360))
    det = Detector(max_scans=T, max_beams=360)
    cnt, mk = det.detect(scans, np.zeros(T), np.full(T, inc))
    det.close()
    c = np.clip(cnt, 0, mk.shape[1])
    keep = np.arange(mk.shape[1])[None, :] < c[:, None]
    rel = np.stack([np.where(keep, mk["x"], 0.0), np.where(keep, mk["y"], 0.0)], -1)
    scg = synth.Scenario(sc.n_landmarks, sc.landmarks, sc.wheel, np.full(keep.shape, -1, np.int32),
                         np.zeros(keep.shape, np.int32), rel, c.astype(np.int32), sc.truth,
                         sc.track, sc.radius)
    corr = int(c.sum())
    s = pyekf.Slam(n_landmarks=50, source=pyekf.SOURCE_ASSOC)
    times = {False: [], True: []}
    out = {}
    for r in range(reps + 1):
        for trace in (False, True):
            s.reset()
            t0 = time.perf_counter()
            _, poses, tmo = s.replay(scg, poses=True, trace=trace)
            dt = time.perf_counter() - t0
            out[trace] = (poses, tmo)
            if r:
                times[trace].append(dt)
    s.close()
    return {"scans": T, "corrections": corr,
            "per_message_sync_ms": med(times[False]) * 1e3,
            "trace_ms": med(times[True]) * 1e3,
            "per_message_sync_corrections_per_s": corr / med(times[False]),
            "trace_corrections_per_s": corr / med(times[True]),
            "max_abs_pose_difference": float(np.abs(out[True][0] - out[False][0]).max()),
            "max_abs_map_odom_difference": float(np.abs(out[True][1] - out[False][1]).max()),
            "per_message_sync_ms_all": [t * 1e3 for t in times[False]],
            "trace_ms_all": [t * 1e3 for t in times[True]]}


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--reps", type=int, default=5)
    p.add_argument("--out", default=None)
    a = p.parse_args()
    res = {"reps": a.reps, "n1024_fp32": headline(a.reps), "basic_world": basic_world(a.reps),
           "surrogate": surrogate(a.reps)}
    txt = json.dumps(res, indent=1)
    print(txt)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(txt + "\n")


if __name__ == "__main__":
    main()
