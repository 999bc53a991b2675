"""Dev tool: ekf_copy_state (the device route) against the host route it replaces.

The host route is the only way before ekf_copy_state: per filter ekf_get_state + ekf_get_map_odom on
the source, ekf_set_state + ekf_set_odom on the destination, every Σ over PCIe and through two host
n² loops (for a fork the source is read once and set into every destination filter). Both routes
are timed as the wall time of a call sequence that ends synchronised (ekf_copy_state synchronises
itself, the host route ends in ekf_sync), taken in turn, and reported as median with min / max.

Shapes:
  swarm   512 filters of N = 256, fp64 -> fp64, filter f onto filter f
  fork    one filter of N = 256 into 512, fp64 -> fp64
  one     one filter of N = 1024, fp64 pipeline -> fp32

The device route's bytes/s are over its algorithmic bytes: every source Σ (n² elements) read once,
every destination Σ written once. Before timing, both routes' results are compared bit for bit on
the first and the last destination filter. Prints one JSON line per shape.

  python tools/copy_state_bench.py [--reps 20] [--host-reps 5] [--warmup 2] [--shapes swarm fork one]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ekf-slam_amd"))
import pyekf  # noqa: E402

SHAPES = {  # N, source filters, destination filters, destination dtype, fork
    "swarm": (256, 512, 512, pyekf.EKF_F64, False),
    "fork": (256, 1, 512, pyekf.EKF_F64, True),
    "one": (1024, 1, 1, pyekf.EKF_F32, False),
}


def spread(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v), "reps": len(v)}


def fill(src, rng):
    """A dense symmetric Σ and a state in every source filter (what is copied does not matter to
    the time; the comparison below wants more than Σ₀)."""
    n = src.n
    a = rng.normal(size=(n, n)) * 1e-2
    S = a @ a.T + np.eye(n)
    for f in range(src.F):
        src.set_state(rng.normal(size=n), S * (1.0 + f), tmo=rng.normal(size=3), counter=f + 1, f=f)
        src.set_odom(rng.normal(size=3), f)


def host_route(dst, src, fork, buf):
    L = pyekf.lib()
    x, S, tmo, cnt = buf
    for fd in range(dst.F):
        if fd == 0 or not fork:
            fs = 0 if fork else fd
            L.ekf_get_state(src.h, fs, x.ctypes.data, S.ctypes.data, C.byref(cnt))
            L.ekf_get_map_odom(src.h, fs, tmo.ctypes.data)
        L.ekf_set_state(dst.h, fd, x.ctypes.data, S.ctypes.data, tmo.ctypes.data, cnt.value)
        L.ekf_set_odom(dst.h, fd, 0.0, 0.0, 0.0)
    dst.sync()


def device_route(dst, src, fork):
    dst.copy_state_from(src, 0 if fork else None)


def timed(fn, *a):
    t0 = time.perf_counter()
    fn(*a)
    return time.perf_counter() - t0


def run(name, reps, host_reps, warmup):
    N, Fs, Fd, dtype, fork = SHAPES[name]
    rng = np.random.default_rng(3)
    src = pyekf.EKF(N, Fs, pyekf.EKF_F64)
    dev, host = pyekf.EKF(N, Fd, dtype), pyekf.EKF(N, Fd, dtype)
    assert src.path == dev.path == pyekf.EKF_PATH_PIPELINE
    fill(src, rng)
    buf = (np.zeros(src.n), np.zeros((src.n, src.n)), np.zeros(3), C.c_uint(0))
    device_route(dev, src, fork)
    host_route(host, src, fork, buf)
    for f in (0, Fd - 1):
        for a, b in zip(dev.state(f), host.state(f)):
            assert np.array_equal(a, b), (name, f)
        assert np.array_equal(dev.map_odom(f), host.map_odom(f)), (name, f)
    for _ in range(warmup):
        device_route(dev, src, fork)
    t_dev, t_host = [], []
    for r in range(max(reps, host_reps)):
        if r < reps:
            t_dev.append(timed(device_route, dev, src, fork))
        if r < host_reps:
            t_host.append(timed(host_route, host, src, fork, buf))
    n = src.n
    nbytes = n * n * 8 * (1 if fork else Fs) + n * n * (4 if dtype == pyekf.EKF_F32 else 8) * Fd
    d, h = spread(t_dev), spread(t_host)
    out = {"shape": name, "N": N, "src_filters": Fs, "dst_filters": Fd,
           "dst_dtype": "f32" if dtype == pyekf.EKF_F32 else "f64",
           "device_s": d, "host_s": h, "algorithmic_bytes": nbytes,
           "device_bytes_per_s": nbytes / d["median"],
           "host_over_device": h["median"] / d["median"]}
    print(json.dumps(out), flush=True)
    for e in (src, dev, host):
        e.close()
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--host-reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--shapes", nargs="+", default=list(SHAPES), choices=list(SHAPES))
    a = ap.parse_args()
    for name in a.shapes:
        run(name, a.reps, a.host_reps, a.warmup)


if __name__ == "__main__":
    main()
