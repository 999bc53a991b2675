"""Example: a Monte-Carlo swarm with unknown association, run and scored without its inputs or its
truth visiting the host.

  Sim.run_assoc   simulates the wheels and the fake sensor on the GPU and hands the markers, ids
                  ignored, to the device-input association replay (ekf_sim_run_assoc)
  Sim.eval_match  matches the slots each filter opened to its true map on the device and scores
                  them (ekf_sim_eval_match)

Prints one JSON line: ekf_eval_summary of the records plus the association's quality summed over
the swarm — duplicate slots (n_dup), slots near no landmark (n_spurious) and landmarks never mapped
(n_missed). An example, not a benchmark: nothing is timed.

  python tools/mc_assoc.py [--filters 64] [--landmarks 50] [--messages 40] [--max-dist 0.3]

--kernel-times instead prints the device times of k_eval and k_eval_match (ekf_profile_read kinds 5
and 6: HIP events carried by the dispatches) on one handle of --filters filters with
N = n_map = --landmarks in fp32, every slot seen and the truth a shuffled copy of the slots:
the median of --reps launches each after --warmup untimed ones.

  python tools/mc_assoc.py --kernel-times --filters 64 --landmarks 1024
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ekf-slam_amd"))
import pyekf  # noqa: E402
from pyekf import synth  # noqa: E402


def monte_carlo(a):
    sw = synth.swarm(a.landmarks, a.filters, a.messages, seed=a.seed, survey=False)
    e = pyekf.EKF(n_landmarks=a.landmarks, n_filters=a.filters)
    sim = pyekf.Sim(e, sw.landmarks, seed=int(sw.seeds[0]), ticks_per_msg=sw.wheel.shape[1],
                    max_markers=min(16, sw.landmarks.shape[1]), marker_stride=sw.ids.shape[2],
                    start_theta=sw.start_pose[0], start_x=sw.start_pose[1],
                    start_y=sw.start_pose[2])
    sim.run_assoc(sw.cmd)
    recs, mrecs, _ = sim.eval_match(a.max_dist)
    out = {"filters": a.filters, "N": a.landmarks, "messages": a.messages,
           "max_dist": a.max_dist, "path": "resident" if e.path else "pipeline"}
    out.update(pyekf.eval_summary(recs))
    for k in ("n_truth", "n_matched", "n_primary", "n_dup", "n_spurious", "n_missed"):
        out[k] = int(mrecs[k].sum())
    out["max_match_dist"] = float(mrecs["max_match_dist"].max())
    sim.close()
    e.close()
    print(json.dumps(out), flush=True)


def kernel_times(a):
    F, N = a.filters, a.landmarks
    rng = np.random.default_rng(a.seed)
    e = pyekf.EKF(n_landmarks=N, n_filters=F, dtype=pyekf.EKF_F32)
    half = 0.5 * np.sqrt(N)
    pose = np.zeros((F, 3))
    slots = rng.uniform(-half, half, (F, N, 2))
    perm = np.stack([rng.permutation(N) for _ in range(F)])
    for f in range(F):
        e.set_state(np.concatenate([[0.0, 0.0, 0.0], slots[f].reshape(-1)]), counter=N, f=f)
    in_order = slots + rng.normal(size=slots.shape) * 0.01
    shuffled = np.stack([in_order[f, perm[f]] for f in range(F)])
    e.profile(True)
    ms = {5: [], 6: []}
    for i in range(a.warmup + a.reps):
        e.eval(pose, in_order)
        got = e.eval_match(pose, shuffled, a.max_dist)
        for kind in (5, 6):
            n, t = e.profile_read(kind)
            assert n == 1, (kind, n)
            if i >= a.warmup:
                ms[kind].append(t)
    assert (got[1]["n_matched"] == N).all()   # every slot found its landmark
    out = {"filters": F, "N": N, "n_map": N, "dtype": "f32", "reps": a.reps}
    for kind, name in ((5, "k_eval"), (6, "k_eval_match")):
        out[name] = {"us_median": 1e3 * statistics.median(ms[kind]), "us_min": 1e3 * min(ms[kind]),
                     "us_max": 1e3 * max(ms[kind])}
    e.close()
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--filters", type=int, default=64)
    ap.add_argument("--landmarks", type=int, default=50)
    ap.add_argument("--messages", type=int, default=40)
    ap.add_argument("--max-dist", type=float, default=0.3)
    ap.add_argument("--seed", type=int, default=20240317)
    ap.add_argument("--kernel-times", action="store_true")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    (kernel_times if a.kernel_times else monte_carlo)(a)


if __name__ == "__main__":
    main()
