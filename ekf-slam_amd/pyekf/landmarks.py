"""ctypes wrapper of include/landmarks.h — the lidar landmark front-end (nuslam/src/landmarks.cpp,
turtlelib/src/landmark_detection.cpp) and the simulated laser that can feed it
(nusim/src/nusim.cpp:559-710) on the GPU. Plumbing for tests and bench.py."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import EKF_OK, EkfError, ScanConfig, lib

LM_MAX_BEAMS, LM_MAX_CLUSTER, LM_NO_BREAK = 2048, 39, -1
LM_MAX_CIRCLES = 1024
MARKER_DTYPE = np.dtype([("x", "<f8"), ("y", "<f8"), ("r", "<f8"), ("id", "<i4"), ("pad", "<i4")])


def _check(rc, what):
    if rc != EKF_OK:
        raise EkfError(rc, what)


def _clusters(clusters):
    offs = np.zeros(len(clusters) + 1, dtype=np.int32)
    offs[1:] = np.cumsum([len(c) for c in clusters])
    xy = np.ascontiguousarray(np.concatenate([np.asarray(c, dtype=np.float64).reshape(-1, 2)
                                              for c in clusters]), dtype=np.float64)
    return offs, xy


class Detector:
    """Batched Landmarks::laserCallback (landmarks.cpp:109-156): S scans per call."""

    def __init__(self, max_scans=1, max_beams=360, device=0):
        self.h = C.c_void_p()
        self._resident = 0  # scans the last simulate() left on the device
        self._capacity = (max_scans, max_beams)
        _check(lib().lm_create(C.byref(self.h), max_scans, max_beams, device), "lm_create")

    def close(self):
        if self.h:
            lib().lm_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def detect(self, ranges, angle_min, angle_inc, threshold=0.2, max_markers=32):
        """ranges [S, B] float32 → (counts [S], markers [S, max_markers] structured array)."""
        r = np.ascontiguousarray(ranges, dtype=np.float32)
        if r.ndim == 1:
            r = r[None]
        S, B = r.shape
        am = np.ascontiguousarray(np.broadcast_to(np.asarray(angle_min, np.float64), (S,)))
        ai = np.ascontiguousarray(np.broadcast_to(np.asarray(angle_inc, np.float64), (S,)))
        out = np.zeros((S, max_markers), dtype=MARKER_DTYPE)
        cnt = np.zeros(S, dtype=np.int32)
        _check(lib().lm_detect(self.h, S, B, r.ctypes.data, am.ctypes.data, ai.ctypes.data,
                               threshold, out.ctypes.data, max_markers, cnt.ctypes.data),
               "lm_detect")
        return cnt, out

    def markers(self, ranges, angle_min, angle_inc, threshold=0.2, max_markers=32):
        """One scan → list of (id, x, y, r) like the oracle's laser_callback (None: no break)."""
        cnt, out = self.detect(ranges, angle_min, angle_inc, threshold, max_markers)
        if cnt[0] == LM_NO_BREAK:
            return None
        return [(int(m["id"]), float(m["x"]), float(m["y"]), float(m["r"]))
                for m in out[0][:min(int(cnt[0]), max_markers)]]

    def fit_circles(self, clusters):
        offs, xy = _clusters(clusters)
        out = np.zeros((len(clusters), 3))
        _check(lib().lm_fit_circles(self.h, len(clusters), offs.ctypes.data, xy.ctypes.data,
                                    out.ctypes.data), "lm_fit_circles")
        return out

    def check_circles(self, clusters):
        offs, xy = _clusters(clusters)
        out = np.zeros(len(clusters), dtype=np.int32)
        _check(lib().lm_check_circles(self.h, len(clusters), offs.ctypes.data, xy.ctypes.data,
                                      out.ctypes.data), "lm_check_circles")
        return out.astype(bool)

    def simulate(self, poses, circles, scene=None, n_beams=360, ranges=True, **cfg):
        """nusim's simulated laser on the device (lm_simulate): poses [S, 3] = (θ, x, y), circles
        [C, 3] or [G, C, 3] = (x, y, r), scene [S] picks each scan's circle set (None: set 0).
        ``cfg``: lm_scan_config fields (seed, scan0, arena_w, arena_h, range_min, range_max, sigma)
        or ``arena=(w, h)``. The scans stay on the device for ``detect_resident``; returns them as
        float32 [S, n_beams] too unless ``ranges`` is false (then nothing comes back to the host)."""
        p = np.ascontiguousarray(np.atleast_2d(np.asarray(poses, dtype=np.float64)))
        S = p.shape[0]
        c = np.asarray(circles, dtype=np.float64)
        c = np.ascontiguousarray(c.reshape((1, -1, 3)) if c.ndim < 3 else c)
        G, Cn = c.shape[0], c.shape[1]
        sc = None if scene is None else np.ascontiguousarray(scene, dtype=np.int32)
        if sc is not None and sc.shape != (S,):
            raise ValueError("scene must hold one index per scan")
        k = ScanConfig()
        lib().lm_scan_config_default(C.byref(k))
        if "arena" in cfg:
            k.arena_w, k.arena_h = cfg.pop("arena")
        for name, v in cfg.items():
            if name not in dict(ScanConfig._fields_):
                raise TypeError(f"unknown scan setting {name!r}")
            setattr(k, name, v)
        out = np.zeros((S, n_beams), dtype=np.float32) if ranges else None
        _check(lib().lm_simulate(self.h, S, n_beams, p.ctypes.data, G, Cn,
                                 c.ctypes.data if c.size else None,
                                 None if sc is None else sc.ctypes.data, C.byref(k),
                                 None if out is None else out.ctypes.data), "lm_simulate")
        self._resident = S
        self._beams = n_beams
        return out

    def _ran_lidar(self, S, n_beams, max_markers):
        """Sim.run_lidar left S scans and their detect_device results in this handle."""
        self._resident, self._beams = S, n_beams
        self._device = (S, max_markers)

    def fetch_ranges(self):
        """lm_fetch_ranges: the resident scans (the last ``simulate``'s or ``Sim.run_lidar``'s) as
        float32 [S, n_beams] (synchronising)."""
        # (room for whatever the handle can hold: raw calls may have changed what is resident)
        buf = np.zeros(self._capacity[0] * self._capacity[1], dtype=np.float32)
        _check(lib().lm_fetch_ranges(self.h, buf.ctypes.data), "lm_fetch_ranges")
        S, B = self._resident, getattr(self, "_beams", 0)
        return buf[:S * B].reshape(S, B).copy()

    def detect_resident(self, threshold=0.2, max_markers=32):
        """``detect`` on the scans the last ``simulate`` left on the device (lm_detect_resident)."""
        S = max(self._resident, 1)
        out = np.zeros((S, max_markers), dtype=MARKER_DTYPE)
        cnt = np.zeros(S, dtype=np.int32)
        _check(lib().lm_detect_resident(self.h, threshold, out.ctypes.data, max_markers,
                                        cnt.ctypes.data), "lm_detect_resident")
        return cnt, out

    def detect_device(self, ranges=None, angle_min=0.0, angle_inc=0.0, threshold=0.2,
                      max_markers=32):
        """lm_detect_device: ``detect`` whose markers and counts stay on the device (asynchronous).
        ``ranges`` None: on the scans the last ``simulate`` left there. Returns the scan count."""
        if ranges is None:
            S = self._resident
            _check(lib().lm_detect_device(self.h, 0, 0, None, None, None, threshold, max_markers),
                   "lm_detect_device")
        else:
            r = np.ascontiguousarray(ranges, dtype=np.float32)
            if r.ndim == 1:
                r = r[None]
            S, B = r.shape
            am = np.ascontiguousarray(np.broadcast_to(np.asarray(angle_min, np.float64), (S,)))
            ai = np.ascontiguousarray(np.broadcast_to(np.asarray(angle_inc, np.float64), (S,)))
            _check(lib().lm_detect_device(self.h, S, B, r.ctypes.data, am.ctypes.data,
                                          ai.ctypes.data, threshold, max_markers),
                   "lm_detect_device")
        self._device = (S, max_markers)
        return S

    def fetch_markers(self, max_markers=None):
        """lm_fetch_markers: (counts [S], markers [S, max_markers]) of the last ``detect_device``
        (synchronising)."""
        S, cap = getattr(self, "_device", (1, 1))
        mm = cap if max_markers is None else max_markers
        out = np.zeros((S, mm), dtype=MARKER_DTYPE)
        cnt = np.zeros(S, dtype=np.int32)
        _check(lib().lm_fetch_markers(self.h, out.ctypes.data, mm, cnt.ctypes.data),
               "lm_fetch_markers")
        return cnt, out

    def replay_into(self, ekf, T, odom):
        """lm_replay_into: the last ``detect_device``'s scans as T unknown-association messages of
        ``ekf``'s F filters (scan t·F + f is message t of filter f), odom [T, F, 3] on the host.
        Asynchronous on both handles; returns the status code."""
        od = np.ascontiguousarray(odom, dtype=np.float64)
        if od.size != 3 * T * ekf.F:
            raise ValueError("odom must be [T, F, 3]")
        return lib().lm_replay_into(self.h, ekf.h, T, od.ctypes.data)

    def replay_resident(self, ekf, T, odom):
        """lm_replay_resident: ``replay_into`` for a resident filter handle (one kernel launch
        reads the markers in place). Returns the status code."""
        od = np.ascontiguousarray(odom, dtype=np.float64)
        if od.size != 3 * T * ekf.F:
            raise ValueError("odom must be [T, F, 3]")
        return lib().lm_replay_resident(self.h, ekf.h, T, od.ctypes.data)

    def last_simulate_us(self):
        us = C.c_double()
        _check(lib().lm_last_simulate_us(self.h, C.byref(us)), "lm_last_simulate_us")
        return us.value

    def last_kernel_us(self):
        us = C.c_double()
        _check(lib().lm_last_kernel_us(self.h, C.byref(us)), "lm_last_kernel_us")
        return us.value
