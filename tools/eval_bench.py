"""Dev tool: scoring a swarm on the device (ekf_eval) against the only route there was before it, an
ekf_get_state(sigma) loop plus numpy.

Two shapes:
  swarm   512 filters of N = 256, fp64 (one GPU's share of the Monte-Carlo swarm)
  single  one filter of N = 1024, fp32

Every filter gets a state with every landmark slot seen (ekf_set_state, state only) and one
16-marker message, so that its pose block and 16 landmark blocks are a real posterior and the rest
the prior; the truth is drawn near the estimate. What is timed does not depend on the values.

  device  EKF.eval(truth_pose, truth_lm): the truth up (F x (3 + 2N) doubles), one kernel, F x 128
          bytes back.
  host    for every filter EKF.state(f) (the whole n x ld Sigma over PCIe, widened on the host),
          then the same score in vectorised numpy.

Prints one JSON line per shape: the median wall time of --reps calls of each route (each ends in a
device synchronise and the copy back; min / max as the spread) after --warmup untimed ones, the
bytes each route reads from device memory per call, and the largest relative difference between
the two routes' records (a sanity check: tests/test_gpu_eval.py is the test). No ratio is asserted.

  python tools/eval_bench.py [--reps 50] [--host-reps 2] [--warmup 3] [--shape swarm|single]
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

SHAPES = {"swarm": (512, 256, pyekf.EKF_F64), "single": (1, 1024, pyekf.EKF_F32)}
M = 16


def prepare(F, N, dtype, seed=20240317):
    rng = np.random.default_rng(seed)
    e = pyekf.EKF(n_landmarks=N, n_filters=F, dtype=dtype)
    half = 0.5 * np.sqrt(N)
    for f in range(F):
        x = np.concatenate([[0.0, 0.0, 0.0], rng.uniform(-half, half, 2 * N)])
        e.set_state(x, counter=N, f=f)
    ids = np.stack([rng.choice(N, M, replace=False) for _ in range(F)]).astype(np.int32)
    rel = rng.uniform(-2.0, 2.0, (F, M, 2))
    rc = e.batch_sensor(np.full(F, M, np.int32), rel, odom=np.zeros((F, 3)), ids=ids,
                        actions=np.zeros((F, M), np.int32))
    assert rc == pyekf.EKF_OK, rc
    e.sync()
    pose = np.zeros((F, 3))
    lm = np.zeros((F, N, 2))
    for f in range(F):
        x, _, _ = e.state(f, sigma=False)
        pose[f] = x[:3] + rng.normal(size=3) * 0.01
        lm[f] = x[3:].reshape(N, 2) + rng.normal(size=(N, 2)) * 0.05
    return e, pose, lm


def score_numpy(x, S, N, tp, tl):
    """ekf_eval's record of one filter (frame = NULL) in vectorised numpy."""
    r = 3 + 2 * np.arange(N)
    P = 0.5 * (S[:3, :3] + S[:3, :3].T)
    d = np.fmod(x[0] - tp[0] + np.pi, 2 * np.pi)
    err = np.array([d + np.pi if d <= 0 else d - np.pi, x[1] - tp[1], x[2] - tp[2]])
    out = {"pose_err": err, "pose_nees": np.nan}
    try:
        Lc = np.linalg.cholesky(P)
        y = np.linalg.solve(Lc, err)
        out["pose_nees"] = float(y @ y)
    except np.linalg.LinAlgError:
        pass
    xy = np.stack([x[r], x[r + 1]], 1)
    a, b, c = S[r, r], 0.5 * (S[r, r + 1] + S[r + 1, r]), S[r + 1, r + 1]
    seen = (xy != 0).any(1)
    ev = seen & ~np.isnan(tl).any(1)
    dx, dy = (xy - tl)[ev].T
    det = a[ev] * c[ev] - b[ev] ** 2
    pd = (a[ev] > 0) & (det > 0)
    q = (c[ev] * dx * dx - 2 * b[ev] * dx * dy + a[ev] * dy * dy)[pd] / det[pd]
    sq = dx * dx + dy * dy
    out.update(lm_sq_err=float(sq.sum()), lm_nees=float(q.sum()),
               lm_max_err=float(np.sqrt(sq.max())) if sq.size else 0.0,
               lm_var_trace=float((a + c)[seen].sum()), n_seen=int(seen.sum()),
               n_eval=int(ev.sum()), n_nees=int(pd.sum()))
    return out


def timed(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return {"ms_median": 1e3 * statistics.median(ts), "ms_min": 1e3 * min(ts),
            "ms_max": 1e3 * max(ts), "reps": len(ts)}


def run(name, a):
    F, N, dtype = SHAPES[name]
    e, pose, lm = prepare(F, N, dtype)
    w = 4 if dtype == pyekf.EKF_F32 else 8

    def device():
        return e.eval(pose, lm)

    def host():
        return [score_numpy(*e.state(f)[:2], N, pose[f], lm[f]) for f in range(F)]

    dev = timed(device, a.reps, a.warmup)
    hst = timed(host, a.host_reps, 1)
    recs, ref = device(), host()
    worst = 0.0
    for f in range(F):
        for k, v in ref[f].items():
            got = np.asarray(recs[f][k], np.float64)
            v = np.asarray(v, np.float64)
            if np.isnan(v).all() and np.isnan(got).all():
                continue
            worst = max(worst, float(np.max(np.abs(got - v) / np.maximum(np.abs(v), 1e-300))))
    out = {"shape": name, "filters": F, "N": N, "dtype": "f32" if w == 4 else "f64",
           "device": dev, "host": hst,
           # what each route reads of Sigma and x per call: the pose block's three rows of three
           # and 2 x 2 per slot (plus the state), against the whole n x ld Sigma
           "device_bytes_gathered": F * ((9 + 4 * N) * w + e.n * 8),
           "host_bytes_copied": F * (e.n * e.ld * w + e.n * 8),
           "host_over_device": hst["ms_median"] / dev["ms_median"],
           "max_rel_diff_device_vs_numpy": worst}
    e.close()
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--host-reps", type=int, default=2)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--shape", choices=list(SHAPES), action="append")
    a = ap.parse_args()
    for name in a.shape or list(SHAPES):
        run(name, a)


if __name__ == "__main__":
    main()
