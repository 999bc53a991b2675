#!/usr/bin/env python3
"""Device-input replays on the resident path against host-planned ones, per message.

The basic_world drive (4 landmarks in 50 slots, n = 103) for F filters, known ids and unknown
association:
  device  ekf_replay_resident: one launch of k_resident_replay, inputs read from device memory
  host    ekf_replay under ekf_defer: the host plans, uploads once, one launch of k_resident
          (a plan of more than 8192 descriptors goes up in pieces, a launch each)
Per mode: the kernel's own time per message from ekf_profile (slot 4), and the wall time of the
call plus ekf_sync. Medians over --reps runs on a filter reset each time (the first run of each
mode is a warm-up and is dropped). One JSON line per (F, kind); --out appends them to a file.

    python tools/resident_replay_bench.py --filters 1 512 --messages 100 --reps 7
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ekf-slam_amd"))

import numpy as np  # noqa: E402

import pyekf  # noqa: E402
from pyekf import synth  # noqa: E402


def drive(T, F, assoc):
    sc = synth.basic_world(T, shuffle=assoc)
    M = sc.ids.shape[1]
    rep = lambda a: np.ascontiguousarray(np.repeat(a[:, None], F, 1))  # noqa: E731
    od = pyekf.odometry(sc)
    return (rep(sc.count.astype(np.int32)), rep(sc.rel), rep(od), rep(sc.ids.astype(np.int32)),
            rep(sc.actions.astype(np.int32)), M, sc.corrections())


def run(F, T, assoc, reps):
    import torch
    cnt, rel, od, ids, act, M, ncorr = drive(T, F, assoc)
    e = pyekf.EKF(n_landmarks=50, n_filters=F)
    assert e.path == pyekf.EKF_PATH_RESIDENT
    g = [torch.from_numpy(a).cuda() for a in (cnt, rel, od, ids, act)]
    ptr = [t.data_ptr() for t in g]
    torch.cuda.synchronize()
    e.profile(True)
    out = {}
    end = {}
    for mode in ("device", "host"):
        wall, dev = [], []
        for r in range(reps + 1):
            e.reset()
            e.profile_read(4)
            e.defer(mode == "host")
            t0 = time.perf_counter()
            if mode == "device":
                rc = e.replay_resident_raw(int(assoc), T, M, ptr[0], 0 if assoc else ptr[3],
                                           0 if assoc else ptr[4], ptr[1], 2, ptr[2])
                assert rc == pyekf.EKF_OK
            else:
                e.replay(cnt, rel, od, ids=None if assoc else ids,
                         actions=None if assoc else act, assoc=assoc)
            e.sync()
            t1 = time.perf_counter()
            n, ms = e.profile_read(4)
            assert n == 1 or mode == "host", n  # (a large host plan goes up in several launches)
            launches = n
            if r:
                wall.append(1e6 * (t1 - t0) / T)
                dev.append(1e3 * ms / T)
        e.defer(False)
        out[mode] = {"kernel_us_per_msg": round(statistics.median(dev), 3),
                     "kernel_us_min_max": [round(min(dev), 3), round(max(dev), 3)],
                     "wall_us_per_msg": round(statistics.median(wall), 3),
                     "launches": launches}
        end[mode] = e.state(0)
    dx = float(np.abs(end["device"][0] - end["host"][0]).max())
    e.close()
    return {"F": F, "kind": "assoc" if assoc else "known", "T": T, "markers_per_msg":
            round(ncorr / T, 2), "reps": reps, **out,
            "kernel_ratio_device_over_host": round(out["device"]["kernel_us_per_msg"] /
                                                   out["host"]["kernel_us_per_msg"], 4),
            "state_diff": dx}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--filters", type=int, nargs="+", default=[1, 512])
    ap.add_argument("--messages", type=int, default=100)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    for F in a.filters:
        for assoc in (False, True):
            line = json.dumps(run(F, a.messages, assoc, a.reps))
            print(line, flush=True)
            if a.out:
                with open(a.out, "a") as fh:
                    fh.write(line + "\n")


if __name__ == "__main__":
    main()
