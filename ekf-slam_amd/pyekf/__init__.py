"""ctypes binding of libekfslam.so (include/ekf.h, include/slam_core.h, include/landmarks.h,
include/ekf_sim.h).

The binding is plumbing for tests and bench.py; the product is the C-ABI library. Loading fails
loudly when the HIP library has not been built — there is no CPU fallback anywhere in this package.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

PKG_DIR = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB_PATH = os.path.join(PKG_DIR, os.environ.get("EKF_LIB", "libekfslam.so"))

EKF_OK, EKF_E_ARG, EKF_E_RANGE, EKF_E_EMPTY, EKF_E_NUMERIC, EKF_E_HIP, EKF_E_NOMEM = \
    0, -1, -2, -3, -4, -5, -6
EKF_E_TIMEOUT = -7
EKF_FLAG_RANGE, EKF_FLAG_NUMERIC, EKF_FLAG_TIMEOUT = 1, 2, 4
EKF_ASSOC_MARKER, EKF_ASSOC_CHUNK, EKF_ASSOC_CHUNK_XCD = 0, 1, 2
EKF_SCHED_DEVSYNC, EKF_SCHED_SERIAL = 1, 4
EKF_SCHED_BUILDER = 2  # deprecated, never set (include/ekf.h)
EKF_F64, EKF_F32 = 0, 1
EKF_PATH_PIPELINE, EKF_PATH_RESIDENT = 0, 1
ADD, DELETE = 0, 2
SOURCE_SIM, SOURCE_ASSOC = 0, 1

# every symbol include/ekf.h and include/slam_core.h declare
EXPORTS = [
    "ekf_config_default", "ekf_strerror", "ekf_create", "ekf_destroy", "ekf_dims", "ekf_get_path",
    "ekf_get_assoc_route", "ekf_get_schedule",
    "ekf_set_odom",
    "ekf_fake_sensor", "ekf_sensor", "ekf_batch_sensor", "ekf_replay", "ekf_replay_device",
    "ekf_replay_device_assoc", "ekf_replay_resident", "ekf_get_decisions",
    "ekf_predict",
    "ekf_correct", "ekf_associate_correct", "ekf_posterior", "ekf_sync", "ekf_flush", "ekf_get_pose",
    "ekf_get_map_odom", "ekf_get_state", "ekf_set_state", "ekf_get_status", "ekf_defer",
    "ekf_set_joseph",
    "ekf_reset", "slam_reset",
    "ekf_trace_enable", "ekf_trace_count", "ekf_trace_read", "ekf_trace_clear", "slam_replay_trace",
    "ekf_profile_enable", "ekf_profile_read", "ekf_sigma_pass_bytes", "ekf_chain_path_counts",
    "ekf_normalize_angle", "ekf_debug_poison_lds",
    "slam_create", "slam_destroy", "slam_joint_states", "slam_markers", "slam_initial_pose",
    "slam_odom", "slam_map_odom", "slam_filter", "slam_replay", "slam_integrate_odometry",
    "lm_create", "lm_destroy", "lm_detect", "lm_fit_circles", "lm_check_circles",
    "lm_last_kernel_us",
    "lm_scan_config_default", "lm_simulate", "lm_detect_resident", "lm_last_simulate_us",
    "lm_detect_device", "lm_fetch_markers", "lm_replay_into", "lm_replay_resident",
    "ekf_sim_config_default", "ekf_sim_create", "ekf_sim_destroy", "ekf_sim_run",
    "ekf_sim_markers", "ekf_sim_poses",
    "ekf_get_marginals", "ekf_eval", "ekf_eval_summary", "ekf_sim_eval",
    "ekf_eval_match", "ekf_sim_run_assoc", "ekf_sim_eval_match",
    "ekf_sim_lidar_config_default", "ekf_sim_run_lidar", "lm_fetch_ranges",
    "ekf_sim_set_collisions", "ekf_sim_collisions", "ekf_sim_last_us",
    "ekf_copy_state", "ekf_sim_fork",
]
TRACE_EXPORTS = ("ekf_trace_enable", "ekf_trace_count", "ekf_trace_read", "ekf_trace_clear",
                 "slam_replay_trace")
# what a library built from an earlier commit (EKF_LIB, the A/B tools) may lack
EVAL_EXPORTS = ("ekf_get_marginals", "ekf_eval", "ekf_eval_summary", "ekf_sim_eval")
MATCH_EXPORTS = ("ekf_eval_match", "ekf_sim_run_assoc", "ekf_sim_eval_match")
LIDAR_EXPORTS = ("ekf_sim_lidar_config_default", "ekf_sim_run_lidar", "lm_fetch_ranges")
COLLIDE_EXPORTS = ("ekf_sim_set_collisions", "ekf_sim_collisions")
SIM_DEV_EXPORTS = ("ekf_sim_last_us",)  # measurement hook (EKF_SIM_TIMING), not part of the feature
COPY_EXPORTS = ("ekf_copy_state", "ekf_sim_fork")
LATER_EXPORTS = (TRACE_EXPORTS + ("ekf_replay_resident", "lm_replay_resident") + EVAL_EXPORTS +
                 MATCH_EXPORTS + ("ekf_chain_path_counts",) + LIDAR_EXPORTS + COLLIDE_EXPORTS +
                 SIM_DEV_EXPORTS + COPY_EXPORTS)
EKF_MATCH_MAX_MAP = 1024
EKF_EVAL_POSE_NOT_PD, EKF_EVAL_LM_NOT_PD = 1, 2
SENSE_NEAREST, SENSE_SURVEY, SENSE_ALL = 0, 1, 2


class EkfError(RuntimeError):
    def __init__(self, rc: int, what: str = ""):
        self.rc = rc
        super().__init__(f"{what}: {lib().ekf_strerror(rc).decode()} ({rc})")


class SimConfig(C.Structure):
    _fields_ = [("seed", C.c_ulonglong), ("f0", C.c_int), ("ticks_per_msg", C.c_int),
                ("slip", C.c_double), ("sensor_sigma", C.c_double), ("max_range", C.c_double),
                ("max_markers", C.c_int), ("marker_stride", C.c_int),
                ("wheel_radius", C.c_double), ("track_width", C.c_double),
                ("start_theta", C.c_double), ("start_x", C.c_double), ("start_y", C.c_double),
                ("record", C.c_int)]


class ScanConfig(C.Structure):
    """lm_scan_config (include/landmarks.h)."""
    _fields_ = [("seed", C.c_ulonglong), ("scan0", C.c_longlong),
                ("arena_w", C.c_double), ("arena_h", C.c_double),
                ("range_min", C.c_double), ("range_max", C.c_double), ("sigma", C.c_double)]


class LidarConfig(C.Structure):
    """ekf_sim_lidar_config (include/ekf_sim.h)."""
    _fields_ = [("n_beams", C.c_int), ("max_markers", C.c_int), ("threshold", C.c_double),
                ("obstacle_radius", C.c_double), ("scan", ScanConfig)]


class TraceRec(C.Structure):
    """ekf_trace_rec (include/ekf.h): one posterior of a filter's pose trace, 64 bytes."""
    _fields_ = [("pose", C.c_double * 3), ("map_odom", C.c_double * 3),
                ("seq", C.c_longlong), ("reserved", C.c_longlong)]


TRACE_DTYPE = np.dtype([("pose", np.float64, 3), ("map_odom", np.float64, 3),
                        ("seq", np.int64), ("reserved", np.int64)])
assert TRACE_DTYPE.itemsize == C.sizeof(TraceRec) == 64


class LmMarginal(C.Structure):
    """ekf_lm_marginal (include/ekf.h): one landmark slot's estimate and 2 x 2 block, 48 bytes."""
    _fields_ = [("xy", C.c_double * 2), ("cov", C.c_double * 3), ("seen", C.c_int),
                ("pad", C.c_int)]


class EvalRec(C.Structure):
    """ekf_eval_rec (include/ekf.h): one filter's score against the truth, 128 bytes."""
    _fields_ = [("pose_err", C.c_double * 3), ("pose_cov", C.c_double * 6),
                ("pose_nees", C.c_double), ("lm_sq_err", C.c_double), ("lm_nees", C.c_double),
                ("lm_max_err", C.c_double), ("lm_var_trace", C.c_double),
                ("n_seen", C.c_int), ("n_eval", C.c_int), ("n_nees", C.c_int),
                ("flags", C.c_uint)]


class MatchRec(C.Structure):
    """ekf_match_rec (include/ekf.h): one filter's association quality, 32 bytes."""
    _fields_ = [("n_truth", C.c_int), ("n_matched", C.c_int), ("n_primary", C.c_int),
                ("n_dup", C.c_int), ("n_spurious", C.c_int), ("n_missed", C.c_int),
                ("max_match_dist", C.c_double)]


class EvalSum(C.Structure):
    """ekf_eval_sum (include/ekf.h): a swarm's records in a few numbers."""
    _fields_ = [("n", C.c_int), ("n_pose_nees", C.c_int), ("anees_pose", C.c_double),
                ("pose_in_95", C.c_double), ("pos_rmse", C.c_double),
                ("heading_rmse", C.c_double), ("lm_rmse", C.c_double), ("anees_lm", C.c_double)]


LM_MARGINAL_DTYPE = np.dtype([("xy", np.float64, 2), ("cov", np.float64, 3), ("seen", np.int32),
                              ("pad", np.int32)])
EVAL_DTYPE = np.dtype([("pose_err", np.float64, 3), ("pose_cov", np.float64, 6),
                       ("pose_nees", np.float64), ("lm_sq_err", np.float64),
                       ("lm_nees", np.float64), ("lm_max_err", np.float64),
                       ("lm_var_trace", np.float64), ("n_seen", np.int32), ("n_eval", np.int32),
                       ("n_nees", np.int32), ("flags", np.uint32)])
assert LM_MARGINAL_DTYPE.itemsize == C.sizeof(LmMarginal) == 48
assert EVAL_DTYPE.itemsize == C.sizeof(EvalRec) == 128
MATCH_DTYPE = np.dtype([("n_truth", np.int32), ("n_matched", np.int32), ("n_primary", np.int32),
                        ("n_dup", np.int32), ("n_spurious", np.int32), ("n_missed", np.int32),
                        ("max_match_dist", np.float64)])
assert MATCH_DTYPE.itemsize == C.sizeof(MatchRec) == 32


class Config(C.Structure):
    _fields_ = [("n_landmarks", C.c_int), ("n_filters", C.c_int), ("dtype", C.c_int),
                ("q_noise", C.c_double), ("r_noise", C.c_double), ("init_var", C.c_double),
                ("mah_gate", C.c_double), ("device", C.c_int)]


_lib = None
_vp, _ip, _dp, _i, _d = C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_double), C.c_int, C.c_double


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(f"{LIB_PATH} is missing: build it with `make -C {PKG_DIR}` "
                               "(or __graft_entry__.build()); there is no CPU fallback")
        L = C.CDLL(LIB_PATH, mode=C.RTLD_GLOBAL)
        sig = {
            "ekf_config_default": (None, [C.POINTER(Config)]),
            "ekf_strerror": (C.c_char_p, [_i]),
            "ekf_create": (_i, [C.POINTER(_vp), C.POINTER(Config)]),
            "ekf_destroy": (_i, [_vp]),
            "ekf_dims": (_i, [_vp, _ip, _ip, _ip]),
            "ekf_get_path": (_i, [_vp, _ip]),
            "ekf_get_assoc_route": (_i, [_vp, _ip]),
            "ekf_get_schedule": (_i, [_vp, _ip]),
            "ekf_set_odom": (_i, [_vp, _i, _d, _d, _d]),
            "ekf_fake_sensor": (_i, [_vp, _i, _i, _vp, _vp, _vp]),
            "ekf_sensor": (_i, [_vp, _i, _i, _vp, _vp, _vp]),
            "ekf_batch_sensor": (_i, [_vp, _i, _i, _vp, _vp, _vp, _vp, _vp]),
            "ekf_replay": (_i, [_vp, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp]),
            "ekf_replay_device": (_i, [_vp, _i, _i, _vp, _vp, _vp, _vp, _vp]),
            "ekf_replay_device_assoc": (_i, [_vp, _i, _i, _vp, _vp, _i, _vp]),
            "ekf_replay_resident": (_i, [_vp, _i, _i, _i, _vp, _vp, _vp, _vp, _i, _vp]),
            "ekf_get_decisions": (_i, [_vp, _i, _i, _vp, _vp]),
            "ekf_predict": (_i, [_vp, _i]),
            "ekf_correct": (_i, [_vp, _i, _i, _d, _d]),
            "ekf_associate_correct": (_i, [_vp, _i, _d, _d, _ip, _ip]),
            "ekf_posterior": (_i, [_vp, _i]),
            "ekf_sync": (_i, [_vp]),
            "ekf_flush": (_i, [_vp]),
            "ekf_get_pose": (_i, [_vp, _i, _vp]),
            "ekf_get_map_odom": (_i, [_vp, _i, _vp]),
            "ekf_get_state": (_i, [_vp, _i, _vp, _vp, _vp]),
            "ekf_set_state": (_i, [_vp, _i, _vp, _vp, _vp, C.c_uint]),
            "ekf_get_status": (_i, [_vp, _i, C.POINTER(C.c_uint)]),
            "ekf_defer": (_i, [_vp, _i]),
            "ekf_set_joseph": (_i, [_vp, _i]),
            "ekf_reset": (_i, [_vp, _i]),
            "slam_reset": (_i, [_vp]),
            "ekf_trace_enable": (_i, [_vp, _i]),
            "ekf_chain_path_counts": (_i, [_vp, _i, C.POINTER(C.c_ulonglong),
                                           C.POINTER(C.c_ulonglong)]),
            "ekf_trace_count": (_i, [_vp, _i, C.POINTER(C.c_longlong)]),
            "ekf_trace_read": (_i, [_vp, _i, C.c_longlong, _i, _vp, _ip]),
            "ekf_trace_clear": (_i, [_vp, _i]),
            "slam_replay_trace": (_i, [_vp, _i, _i, _vp, _i, _vp, _vp, _vp, _vp, _vp, _vp]),
            "ekf_profile_enable": (_i, [_vp, _i]),
            "ekf_profile_read": (_i, [_vp, _i, C.POINTER(C.c_longlong), _dp]),
            "ekf_sigma_pass_bytes": (C.c_double, [_vp, _i]),
            "ekf_normalize_angle": (C.c_double, [_d]),
            "ekf_debug_poison_lds": (_i, [_i]),
            "slam_create": (_i, [C.POINTER(_vp), C.POINTER(Config), _d, _d, _i]),
            "slam_destroy": (_i, [_vp]),
            "slam_joint_states": (_i, [_vp, _d, _d]),
            "slam_markers": (_i, [_vp, _i, _vp, _vp, _vp]),
            "slam_initial_pose": (_i, [_vp, _d, _d, _d]),
            "slam_odom": (_i, [_vp, _vp]),
            "slam_map_odom": (_i, [_vp, _vp]),
            "slam_filter": (_vp, [_vp]),
            "slam_replay": (_i, [_vp, _i, _i, _vp, _i, _vp, _vp, _vp, _vp, _vp, _vp]),
            "slam_integrate_odometry": (_i, [_d, _d, _i, _i, _vp, _vp]),
            "lm_create": (_i, [C.POINTER(_vp), _i, _i, _i]),
            "lm_destroy": (_i, [_vp]),
            "lm_detect": (_i, [_vp, _i, _i, _vp, _vp, _vp, _d, _vp, _i, _vp]),
            "lm_fit_circles": (_i, [_vp, _i, _vp, _vp, _vp]),
            "lm_check_circles": (_i, [_vp, _i, _vp, _vp, _vp]),
            "lm_last_kernel_us": (_i, [_vp, _dp]),
            "lm_scan_config_default": (None, [C.POINTER(ScanConfig)]),
            "lm_simulate": (_i, [_vp, _i, _i, _vp, _i, _i, _vp, _vp, C.POINTER(ScanConfig), _vp]),
            "lm_detect_resident": (_i, [_vp, _d, _vp, _i, _vp]),
            "lm_last_simulate_us": (_i, [_vp, _dp]),
            "lm_detect_device": (_i, [_vp, _i, _i, _vp, _vp, _vp, _d, _i]),
            "lm_fetch_markers": (_i, [_vp, _vp, _i, _vp]),
            "lm_replay_into": (_i, [_vp, _vp, _i, _vp]),
            "lm_replay_resident": (_i, [_vp, _vp, _i, _vp]),
            "ekf_sim_config_default": (None, [C.POINTER(SimConfig)]),
            "ekf_sim_create": (_i, [C.POINTER(_vp), _vp, C.POINTER(SimConfig), _i, _vp]),
            "ekf_sim_destroy": (_i, [_vp]),
            "ekf_sim_run": (_i, [_vp, _i, _vp, _vp]),
            "ekf_sim_markers": (_i, [_vp, _vp, _vp, _vp, _vp]),
            "ekf_sim_poses": (_i, [_vp, _vp, _vp]),
            "ekf_get_marginals": (_i, [_vp, _i, _vp, _vp, _vp, _vp]),
            "ekf_eval": (_i, [_vp, _vp, _vp, _i, _vp, _vp]),
            "ekf_eval_summary": (_i, [_vp, _i, C.POINTER(EvalSum)]),
            "ekf_sim_eval": (_i, [_vp, _vp]),
            "ekf_eval_match": (_i, [_vp, _vp, _vp, _i, _vp, _d, _vp, _vp, _vp]),
            "ekf_sim_run_assoc": (_i, [_vp, _i, _vp]),
            "ekf_sim_eval_match": (_i, [_vp, _d, _vp, _vp, _vp]),
            "ekf_sim_lidar_config_default": (None, [C.POINTER(LidarConfig)]),
            "ekf_sim_run_lidar": (_i, [_vp, _vp, _i, _vp, C.POINTER(LidarConfig)]),
            "lm_fetch_ranges": (_i, [_vp, _vp]),
            "ekf_sim_set_collisions": (_i, [_vp, _d, _d]),
            "ekf_sim_collisions": (_i, [_vp, _vp, _vp]),
            "ekf_sim_last_us": (_i, [_vp, _dp]),
            "ekf_copy_state": (_i, [_vp, _i, _vp, _i]),
            "ekf_sim_fork": (_i, [_vp, _vp, _i]),
        }
        for name, (res, argt) in sig.items():
            # (EKF_LIB naming a library built from an earlier commit, for the A/B tools: it loads
            # without the pose trace, the resident device replays, the scoring or the matching, and a
            # call of one fails;
            # build() checks EXPORTS)
            if name in LATER_EXPORTS and not hasattr(L, name):
                continue
            fn = getattr(L, name)
            fn.restype = res
            fn.argtypes = argt
        _lib = L
    return _lib


def _ptr(a):
    return None if a is None else a.ctypes.data


def _dptr(x, dtype):
    """A device buffer for ekf_replay_device: None, an int address, or a contiguous torch tensor
    of the given dtype on the GPU."""
    if x is None or isinstance(x, int):
        return x
    if not (x.is_cuda and x.is_contiguous() and x.dtype == dtype):
        raise ValueError(f"device input must be a contiguous {dtype} GPU tensor")
    return x.data_ptr()


def _f64(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def _i32(a):
    return np.ascontiguousarray(a, dtype=np.int32)


def make_config(n_landmarks=50, n_filters=1, dtype=EKF_F64, q_noise=1e-2, r_noise=1e-2,
                init_var=10e6, mah_gate=2.0, device=0) -> Config:
    c = Config()
    lib().ekf_config_default(C.byref(c))
    c.n_landmarks, c.n_filters, c.dtype = n_landmarks, n_filters, dtype
    c.q_noise, c.r_noise, c.init_var, c.mah_gate, c.device = (q_noise, r_noise, init_var,
                                                             mah_gate, device)
    return c


def _check(rc, what):
    if rc != EKF_OK:
        raise EkfError(rc, what)
    return rc


class EKF:
    """A handle of F independent filters (F = 1: one slam node's filter)."""

    def __init__(self, n_landmarks=50, n_filters=1, dtype=EKF_F64, **kw):
        self.cfg = make_config(n_landmarks, n_filters, dtype, **kw)
        h = C.c_void_p()
        _check(lib().ekf_create(C.byref(h), C.byref(self.cfg)), "ekf_create")
        self.h = h
        n, ld, nf = C.c_int(), C.c_int(), C.c_int()
        lib().ekf_dims(self.h, C.byref(n), C.byref(ld), C.byref(nf))
        self.n, self.ld, self.F = n.value, ld.value, nf.value
        self.N = n_landmarks
        p = C.c_int()
        _check(lib().ekf_get_path(self.h, C.byref(p)), "ekf_get_path")
        self.path = p.value  # EKF_PATH_PIPELINE | EKF_PATH_RESIDENT
        _check(lib().ekf_get_assoc_route(self.h, C.byref(p)), "ekf_get_assoc_route")
        self.assoc_route = p.value  # EKF_ASSOC_*
        _check(lib().ekf_get_schedule(self.h, C.byref(p)), "ekf_get_schedule")
        self.schedule = p.value  # EKF_SCHED_* bits

    def close(self):
        if getattr(self, "h", None):
            lib().ekf_destroy(self.h)
            self.h = None

    __del__ = close

    # callbacks
    def set_odom(self, pose, f=0):
        return lib().ekf_set_odom(self.h, f, float(pose[0]), float(pose[1]), float(pose[2]))

    def fake_sensor(self, ids, actions, rel_xy, f=0) -> int:
        ids, act, rel = _i32(ids), _i32(actions), _f64(rel_xy)
        return lib().ekf_fake_sensor(self.h, f, len(ids), _ptr(ids), _ptr(act), _ptr(rel))

    def sensor(self, rel_xy, f=0, decisions=True):
        rel = _f64(rel_xy)
        m = rel.size // 2
        j = np.zeros(max(m, 1), np.int32)
        nw = np.zeros(max(m, 1), np.int32)
        rc = lib().ekf_sensor(self.h, f, m, _ptr(rel), _ptr(j) if decisions else None,
                              _ptr(nw) if decisions else None)
        return rc, j[:m], nw[:m]

    def batch_sensor(self, counts, rel_xy, odom=None, ids=None, actions=None, assoc=False):
        counts, rel = _i32(counts), _f64(rel_xy)
        m_max = rel.shape[1]
        ids = None if ids is None else _i32(ids)
        actions = None if actions is None else _i32(actions)
        odom = None if odom is None else _f64(odom)
        return lib().ekf_batch_sensor(self.h, int(assoc), m_max, _ptr(counts), _ptr(ids),
                                      _ptr(actions), _ptr(rel), _ptr(odom))

    def replay(self, counts, rel_xy, odom, ids=None, actions=None, assoc=False, poses=False):
        """counts[T][F], rel_xy[T][F][M][2], odom[T][F][3]."""
        counts, rel, odom = _i32(counts), _f64(rel_xy), _f64(odom)
        T, M = rel.shape[0], rel.shape[2]
        ids = None if ids is None else _i32(ids)
        actions = None if actions is None else _i32(actions)
        out = np.zeros((T, self.F, 3)) if poses else None
        rc = lib().ekf_replay(self.h, int(assoc), T, M, _ptr(counts), _ptr(ids), _ptr(actions),
                              _ptr(rel), _ptr(odom), _ptr(out))
        _check(rc, "ekf_replay")
        return out

    def replay_device(self, counts, rel_xy, odom, ids, actions=None):
        """ekf_replay_device: known-id replay whose inputs are GPU tensors already on this handle's
        device — counts [T,F] int32, rel_xy [T,F,M,2] float64, odom [T,F,3] float64, ids / actions
        [T,F,M] int32 (M <= EKF_MAX_CHUNK). Asynchronous; keep the tensors alive until a sync."""
        import torch
        T, M = int(rel_xy.shape[0]), int(rel_xy.shape[2])
        rc = lib().ekf_replay_device(self.h, T, M, _dptr(counts, torch.int32),
                                     _dptr(ids, torch.int32), _dptr(actions, torch.int32),
                                     _dptr(rel_xy, torch.float64), _dptr(odom, torch.float64))
        _check(rc, "ekf_replay_device")

    def replay_device_raw(self, T, M, counts, rel_xy, odom, ids, actions=0):
        """ekf_replay_device on raw device addresses (ints: the same layouts as replay_device):
        no tensor work on the caller's path (bench.py's timed region)."""
        _check(lib().ekf_replay_device(self.h, T, M, counts, ids, actions or None, rel_xy, odom),
               "ekf_replay_device")

    def replay_device_assoc(self, counts, xy, odom, stride=None):
        """ekf_replay_device_assoc: unknown-association replay whose inputs are GPU tensors already
        on this handle's device — counts [T,F] int32 (<= 0: no message), xy [T,F,M,2] float64
        (packed pairs) or [T,F,M,4] (lm_marker rows: x, y first), odom [T,F,3] float64; M <= 64.
        ``stride``: doubles between markers, by default xy.shape[-1]. Asynchronous; keep the
        tensors alive until a sync."""
        import torch
        T, M = int(xy.shape[0]), int(xy.shape[2])
        stride = int(xy.shape[-1]) if stride is None else int(stride)
        if stride not in (2, 4):
            raise ValueError("xy must hold 2 (packed) or 4 (lm_marker) doubles per marker")
        _check(lib().ekf_replay_device_assoc(self.h, T, M, _dptr(counts, torch.int32),
                                             _dptr(xy, torch.float64), stride,
                                             _dptr(odom, torch.float64)),
               "ekf_replay_device_assoc")

    def replay_device_assoc_raw(self, T, M, counts, xy, stride, odom):
        """ekf_replay_device_assoc on raw device addresses (ints); returns the status code."""
        return lib().ekf_replay_device_assoc(self.h, T, M, counts or None, xy or None, stride,
                                             odom or None)

    def replay_resident(self, counts, xy, odom, ids=None, actions=None, stride=None):
        """ekf_replay_resident: a replay on a resident handle whose inputs are GPU tensors already
        on this handle's device, run by one kernel launch — counts [T,F] int32 (<= 0: no message),
        xy [T,F,M,2] float64 (packed pairs) or [T,F,M,4] (lm_marker rows: x, y first), odom [T,F,3]
        float64; M <= 64. ``ids`` [T,F,M] int32 (and optionally ``actions``): known ids; ``ids``
        None: unknown association. ``stride``: doubles between markers, by default xy.shape[-1].
        Asynchronous; keep the tensors alive until a sync."""
        import torch
        T, M = int(xy.shape[0]), int(xy.shape[2])
        stride = int(xy.shape[-1]) if stride is None else int(stride)
        rc = self.replay_resident_raw(int(ids is None), T, M, _dptr(counts, torch.int32),
                                      _dptr(ids, torch.int32), _dptr(actions, torch.int32),
                                      _dptr(xy, torch.float64), stride,
                                      _dptr(odom, torch.float64))
        _check(rc, "ekf_replay_resident")

    def replay_resident_raw(self, assoc, T, M, counts, ids, actions, xy, stride, odom):
        """ekf_replay_resident on raw device addresses (ints, 0 / None: NULL); returns the status
        code."""
        return lib().ekf_replay_resident(self.h, int(assoc), T, M, counts or None, ids or None,
                                         actions or None, xy or None, stride, odom or None)

    def replay_on_device(self, counts, xy, odom, ids=None, actions=None, stride=None):
        """A replay from GPU tensors by whichever entry point this handle's path has: resident
        handles ``replay_resident``; pipeline handles ``replay_device`` (known ``ids``, packed xy,
        M <= 16) or ``replay_device_assoc`` (``ids`` None)."""
        if self.path == EKF_PATH_RESIDENT:
            return self.replay_resident(counts, xy, odom, ids=ids, actions=actions, stride=stride)
        if ids is None:
            return self.replay_device_assoc(counts, xy, odom, stride=stride)
        if (int(xy.shape[-1]) if stride is None else int(stride)) != 2:
            raise ValueError("a pipeline handle's known-id replay takes packed (x, y) pairs")
        return self.replay_device(counts, xy, odom, ids, actions)

    def decisions(self, m, f=0):
        """ekf_get_decisions: (assoc [m], is_new [m]) of filter f's most recent unknown-association
        message (m <= 64). Synchronises."""
        j = np.zeros(max(m, 1), np.int32)
        nw = np.zeros(max(m, 1), np.int32)
        _check(lib().ekf_get_decisions(self.h, f, m, _ptr(j), _ptr(nw)), "ekf_get_decisions")
        return j[:m], nw[:m]

    # fine-grained
    def predict(self, f=0):
        return lib().ekf_predict(self.h, f)

    def correct(self, mid, rx, ry, f=0):
        return lib().ekf_correct(self.h, f, int(mid), float(rx), float(ry))

    def associate_correct(self, rx, ry, f=0):
        j, nw = C.c_int(-1), C.c_int(0)
        rc = lib().ekf_associate_correct(self.h, f, float(rx), float(ry), C.byref(j), C.byref(nw))
        return rc, j.value, nw.value

    def posterior(self, f=0):
        return lib().ekf_posterior(self.h, f)

    # state
    def sync(self):
        _check(lib().ekf_sync(self.h), "ekf_sync")

    def flush(self):
        """Submit what is planned, without waiting (ekf_flush)."""
        _check(lib().ekf_flush(self.h), "ekf_flush")

    def pose(self, f=0):
        p = np.zeros(3)
        _check(lib().ekf_get_pose(self.h, f, _ptr(p)), "ekf_get_pose")
        return p

    def map_odom(self, f=0):
        p = np.zeros(3)
        _check(lib().ekf_get_map_odom(self.h, f, _ptr(p)), "ekf_get_map_odom")
        return p

    def state(self, f=0, sigma=True):
        x = np.zeros(self.n)
        S = np.zeros((self.n, self.n)) if sigma else None
        cnt = C.c_uint(0)
        _check(lib().ekf_get_state(self.h, f, _ptr(x), _ptr(S), C.byref(cnt)), "ekf_get_state")
        return x, S, cnt.value

    def set_state(self, state, sigma=None, tmo=None, counter=0, f=0):
        state = _f64(state)
        sigma = None if sigma is None else _f64(sigma)
        tmo = None if tmo is None else _f64(tmo)
        _check(lib().ekf_set_state(self.h, f, _ptr(state), _ptr(sigma), _ptr(tmo), counter),
               "ekf_set_state")

    def copy_state_from(self, src, src_filter=None, dst_filter=None):
        """ekf_copy_state: filter state from the handle ``src`` on the device, as state() on it
        and set_state() + set_odom() here would leave it. src_filter and dst_filter given: one
        filter onto one; src_filter alone: a fork, every filter here receives it; neither: a swarm
        hand-over, filter f receives filter f."""
        _check(lib().ekf_copy_state(self.h, -1 if dst_filter is None else dst_filter, src.h,
                                    -1 if src_filter is None else src_filter), "ekf_copy_state")

    def defer(self, on=True):
        _check(lib().ekf_defer(self.h, int(on)), "ekf_defer")

    def reset(self, f=-1):
        _check(lib().ekf_reset(self.h, f), "ekf_reset")

    def set_joseph(self, on=True) -> int:
        return lib().ekf_set_joseph(self.h, int(on))

    # the pose trace (ekf_trace_*): every message's posterior, recorded on the device
    def trace_enable(self, capacity):
        """Keep up to `capacity` records per filter (0: off and freed). Reallocates and clears."""
        _check(lib().ekf_trace_enable(self.h, int(capacity)), "ekf_trace_enable")

    def chain_path_counts(self, f=0):
        """(lean, generic): corrections the chain kernel's sequential wave has run for filter f in
        its common-case program and in its generic one since the handle's creation or last reset
        (EKF_CHAIN_FAST=0: all of them in the generic one)."""
        a, b = C.c_ulonglong(0), C.c_ulonglong(0)
        _check(lib().ekf_chain_path_counts(self.h, f, C.byref(a), C.byref(b)),
               "ekf_chain_path_counts")
        return a.value, b.value

    def trace_count(self, f=0) -> int:
        """Records appended to filter f's trace (those beyond the capacity are only counted)."""
        n = C.c_longlong(0)
        _check(lib().ekf_trace_count(self.h, f, C.byref(n)), "ekf_trace_count")
        return n.value

    def trace(self, f=0, first=0, n=None):
        """Records [first, first + n) of filter f's trace that are kept (n = None: all from
        `first` on): (pose [k, 3], map_odom [k, 3], seq [k]). Synchronises."""
        if n is None:
            n = max(self.trace_count(f) - first, 0)
        buf = np.zeros(max(n, 1), TRACE_DTYPE)
        got = C.c_int(0)
        _check(lib().ekf_trace_read(self.h, f, first, n, _ptr(buf), C.byref(got)),
               "ekf_trace_read")
        buf = buf[:got.value]
        return buf["pose"].copy(), buf["map_odom"].copy(), buf["seq"].copy()

    def trace_clear(self, f=-1):
        _check(lib().ekf_trace_clear(self.h, f), "ekf_trace_clear")

    # marginals and scoring (ekf_get_marginals, ekf_eval): gathered on the device, read-only
    def marginals(self, f=None):
        """ekf_get_marginals of filter f, or of every filter (f = None: a leading [F] axis):
        (pose [3], pose_cov [3, 3], lm [N] of LM_MARGINAL_DTYPE, counter). Synchronises."""
        lead = (self.F,) if f is None else ()
        pose = np.zeros(lead + (3,))
        cov = np.zeros(lead + (3, 3))
        lm = np.zeros(lead + (self.N,), LM_MARGINAL_DTYPE)
        cnt = np.zeros(lead + (1,), np.uint32)
        _check(lib().ekf_get_marginals(self.h, -1 if f is None else f, _ptr(pose), _ptr(cov),
                                       _ptr(lm), _ptr(cnt)), "ekf_get_marginals")
        return pose, cov, lm, (cnt[..., 0] if f is None else int(cnt[0]))

    def eval(self, truth_pose, truth_lm=None, frame=None):
        """ekf_eval: every filter against truth_pose [F, 3] and truth_lm [F, n_map, 2] (NaN: no
        truth for the slot; None: poses only), frame = (theta0, x0, y0) of the map frame in the
        truth's frame or None. Returns [F] records of EVAL_DTYPE. Synchronises."""
        tp = _f64(truth_pose).reshape(self.F, 3)
        tl = None if truth_lm is None else _f64(truth_lm).reshape(self.F, -1, 2)
        fr = None if frame is None else _f64(frame).reshape(3)
        out = np.zeros(self.F, EVAL_DTYPE)
        _check(lib().ekf_eval(self.h, _ptr(tp), _ptr(tl), 0 if tl is None else tl.shape[1],
                              _ptr(fr), _ptr(out)), "ekf_eval")
        return out

    def eval_match(self, truth_pose, truth_lm, max_dist, frame=None):
        """ekf_eval_match: every filter against truth_pose [F, 3] and a truth map in any order,
        truth_lm [F, n_map, 2] (NaN: no such landmark; n_map <= EKF_MATCH_MAX_MAP): each seen slot
        is matched to its nearest truth landmark within max_dist and scored against it. Returns
        (recs [F] of EVAL_DTYPE, match_recs [F] of MATCH_DTYPE, match [F, N] int32: the slot's
        truth landmark, -1 unseen or unmatched). Synchronises."""
        tp = _f64(truth_pose).reshape(self.F, 3)
        tl = _f64(truth_lm).reshape(self.F, -1, 2)
        fr = None if frame is None else _f64(frame).reshape(3)
        out = np.zeros(self.F, EVAL_DTYPE)
        mrec = np.zeros(self.F, MATCH_DTYPE)
        match = np.full((self.F, self.N), -1, np.int32)
        _check(lib().ekf_eval_match(self.h, _ptr(tp), _ptr(tl), tl.shape[1], _ptr(fr),
                                    float(max_dist), _ptr(out), _ptr(mrec), _ptr(match)),
               "ekf_eval_match")
        return out, mrec, match

    def status(self, f=0) -> int:
        fl = C.c_uint(0)
        _check(lib().ekf_get_status(self.h, f, C.byref(fl)), "ekf_get_status")
        return fl.value

    def profile(self, enable=True):
        lib().ekf_profile_enable(self.h, int(enable))

    def profile_read(self, kernel):
        n, ms = C.c_longlong(0), C.c_double(0)
        _check(lib().ekf_profile_read(self.h, kernel, C.byref(n), C.byref(ms)), "profile_read")
        return n.value, ms.value

    def sigma_pass_bytes(self, filters=None):
        return lib().ekf_sigma_pass_bytes(self.h, self.F if filters is None else filters)


class Slam:
    """slam_core: the reference node's callbacks (include/slam_core.h)."""

    def __init__(self, n_landmarks=50, source=SOURCE_SIM, dtype=EKF_F64, track=0.160,
                 radius=0.033, **kw):
        self.cfg = make_config(n_landmarks, 1, dtype, **kw)
        h = C.c_void_p()
        _check(lib().slam_create(C.byref(h), C.byref(self.cfg), track, radius, source),
               "slam_create")
        self.h = h
        self.n = 3 + 2 * n_landmarks
        p = C.c_int()
        _check(lib().ekf_get_path(lib().slam_filter(self.h), C.byref(p)), "ekf_get_path")
        self.path = p.value

    def close(self):
        if getattr(self, "h", None):
            lib().slam_destroy(self.h)
            self.h = None

    __del__ = close

    def reset(self):
        """A fresh node on the same handle (slam_reset)."""
        _check(lib().slam_reset(self.h), "slam_reset")

    def set_joseph(self, on=True) -> int:
        return lib().ekf_set_joseph(lib().slam_filter(self.h), int(on))

    def profile(self, enable=True):
        lib().ekf_profile_enable(lib().slam_filter(self.h), int(enable))

    def profile_read(self, kernel):
        n, ms = C.c_longlong(0), C.c_double(0)
        _check(lib().ekf_profile_read(lib().slam_filter(self.h), kernel, C.byref(n), C.byref(ms)),
               "profile_read")
        return n.value, ms.value

    def joint_states(self, left, right):
        return lib().slam_joint_states(self.h, float(left), float(right))

    def markers(self, ids, actions, rel_xy):
        rel = _f64(rel_xy)
        ids = None if ids is None else _i32(ids)
        actions = None if actions is None else _i32(actions)
        return lib().slam_markers(self.h, rel.size // 2, _ptr(ids), _ptr(actions), _ptr(rel))

    def initial_pose(self, x, y, theta):
        return lib().slam_initial_pose(self.h, x, y, theta)

    def odom(self):
        p = np.zeros(3)
        lib().slam_odom(self.h, _ptr(p))
        return p

    def map_odom(self):
        p = np.zeros(3)
        _check(lib().slam_map_odom(self.h, _ptr(p)), "slam_map_odom")
        return p

    def filter_state(self, sigma=True):
        ekf = lib().slam_filter(self.h)
        n = self.n
        x = np.zeros(n)
        S = np.zeros((n, n)) if sigma else None
        cnt = C.c_uint(0)
        _check(lib().ekf_get_state(ekf, 0, _ptr(x), _ptr(S), C.byref(cnt)), "ekf_get_state")
        return x, S, cnt.value

    def replay(self, sc, poses=True, trace=False):
        """Drive a synth.Scenario (wheel ticks + marker arrays) natively through the node mirror.
        trace: slam_replay_trace — the drive runs deferred and the per-message outputs come from
        the filter's pose trace."""
        T, ticks = sc.wheel.shape[0], sc.wheel.shape[1]
        M = sc.ids.shape[1]
        wheel, counts = _f64(sc.wheel), _i32(sc.count)
        ids, act, rel = _i32(sc.ids), _i32(sc.actions), _f64(sc.rel)
        out_p = np.zeros((T, 3)) if poses else None
        out_t = np.zeros((T, 3)) if poses else None
        fn = lib().slam_replay_trace if trace else lib().slam_replay
        rc = fn(self.h, T, ticks, _ptr(wheel), M, _ptr(counts), _ptr(ids), _ptr(act), _ptr(rel),
                _ptr(out_p), _ptr(out_t))
        return rc, out_p, out_t


class Sim:
    """ekf_sim_t: on-device Monte-Carlo inputs for an EKF handle (include/ekf_sim.h)."""

    def __init__(self, ekf, landmarks, **cfg):
        c = SimConfig()
        lib().ekf_sim_config_default(C.byref(c))
        for k, v in cfg.items():
            setattr(c, k, v)
        self.cfg = c
        self.F = ekf.F
        self.N = ekf.N
        lm = _f64(np.broadcast_to(np.asarray(landmarks, np.float64),
                                  (ekf.F,) + np.shape(landmarks)[-2:]))
        self.L = lm.shape[1]
        self.h = C.c_void_p()
        _check(lib().ekf_sim_create(C.byref(self.h), ekf.h, C.byref(c), self.L, _ptr(lm)),
               "ekf_sim_create")
        self.T = 0

    def run(self, wheel_cmd, sense=None):
        """wheel_cmd[T·ticks][2] commanded wheel increments per tick; sense[T] or None."""
        cmd = _f64(wheel_cmd).reshape(-1, 2)
        T = cmd.shape[0] // self.cfg.ticks_per_msg
        sn = None if sense is None else _i32(sense)
        _check(lib().ekf_sim_run(self.h, T, _ptr(cmd), _ptr(sn)), "ekf_sim_run")
        self.T = T

    def run_assoc(self, wheel_cmd):
        """ekf_sim_run_assoc: the same simulation (every message senses NEAREST), fed to the filter
        with the ids ignored (unknown association). wheel_cmd[T·ticks][2]."""
        cmd = _f64(wheel_cmd).reshape(-1, 2)
        T = cmd.shape[0] // self.cfg.ticks_per_msg
        _check(lib().ekf_sim_run_assoc(self.h, T, _ptr(cmd)), "ekf_sim_run_assoc")
        self.T = T

    def run_lidar(self, det, wheel_cmd, **cfg):
        """ekf_sim_run_lidar: the same simulation, then the real sensor path on the device — the
        laser scans every (message, filter) from its true pose on the front-end handle ``det``
        (pyekf.landmarks.Detector), which detects on them, and the filter takes the detected markers
        with unknown association. wheel_cmd[T·ticks][2]. ``cfg``: ekf_sim_lidar_config fields
        (n_beams, max_markers, threshold, obstacle_radius), lm_scan_config fields for its ``scan``
        (seed, arena_w, arena_h, range_min, range_max, sigma) or ``arena=(w, h)``."""
        cmd = _f64(wheel_cmd).reshape(-1, 2)
        T = cmd.shape[0] // self.cfg.ticks_per_msg
        c = lidar_config(**cfg)
        _check(lib().ekf_sim_run_lidar(self.h, det.h, T, _ptr(cmd), C.byref(c)),
               "ekf_sim_run_lidar")
        self.T = T
        if T > 0:
            det._ran_lidar(T * self.F, c.n_beams, c.max_markers)

    def fork_from(self, src, src_filter):
        """ekf_sim_fork: every filter of this simulator continues filter ``src_filter`` of the
        simulator ``src`` (which may be this one) under its own seed."""
        _check(lib().ekf_sim_fork(self.h, src.h, src_filter), "ekf_sim_fork")

    def set_collisions(self, collision_radius, obstacle_radius=0.038):
        """ekf_sim_set_collisions: from the next run on the true pose is pushed out of the map's
        cylinders (nusim.cpp:232-254), R = collision_radius + obstacle_radius; 0 turns it off."""
        _check(lib().ekf_sim_set_collisions(self.h, float(collision_radius),
                                            float(obstacle_radius)), "ekf_sim_set_collisions")

    def collisions(self, per_msg=True):
        """ekf_sim_collisions: (total [F] colliding ticks per filter since the simulator was made,
        per_msg [T, F] of the last run; None without ``per_msg``, which needs cfg.record)."""
        total = np.zeros(self.F, np.int64)
        pm = np.zeros((self.T, self.F), np.int32) if per_msg else None
        _check(lib().ekf_sim_collisions(self.h, _ptr(total), _ptr(pm)), "ekf_sim_collisions")
        return total, pm

    def last_us(self):
        """ekf_sim_last_us: µs between the HIP events around the last run's simulator launches (a
        simulator made with EKF_SIM_TIMING=1 in the environment)."""
        us = C.c_double(0.0)
        _check(lib().ekf_sim_last_us(self.h, C.byref(us)), "ekf_sim_last_us")
        return us.value

    def markers(self):
        """The last run's inputs as ekf_replay takes them: counts [T,F], ids/actions [T,F,M],
        rel [T,F,M,2]."""
        T, F, M = self.T, self.F, self.cfg.marker_stride
        cnt = np.zeros((T, F), np.int32)
        ids = np.zeros((T, F, M), np.int32)
        act = np.zeros((T, F, M), np.int32)
        rel = np.zeros((T, F, M, 2))
        _check(lib().ekf_sim_markers(self.h, _ptr(cnt), _ptr(ids), _ptr(act), _ptr(rel)),
               "ekf_sim_markers")
        return cnt, ids, act, rel

    def poses(self):
        """(odom [T, 3], truth [T, F, 3]) of the last run."""
        odom = np.zeros((self.T, 3))
        truth = np.zeros((self.T, self.F, 3))
        _check(lib().ekf_sim_poses(self.h, _ptr(odom), _ptr(truth)), "ekf_sim_poses")
        return odom, truth

    def eval(self):
        """ekf_sim_eval: every filter against the simulator's device-resident truth (its true
        poses, its map, frame = the start pose). Returns [F] records of EVAL_DTYPE."""
        out = np.zeros(self.F, EVAL_DTYPE)
        _check(lib().ekf_sim_eval(self.h, _ptr(out)), "ekf_sim_eval")
        return out

    def eval_match(self, max_dist):
        """ekf_sim_eval_match: EKF.eval_match fed the simulator's device-resident truth (its true
        poses, its map in any order, frame = the start pose). Returns (recs, match_recs, match)."""
        out = np.zeros(self.F, EVAL_DTYPE)
        mrec = np.zeros(self.F, MATCH_DTYPE)
        match = np.full((self.F, self.N), -1, np.int32)
        _check(lib().ekf_sim_eval_match(self.h, float(max_dist), _ptr(out), _ptr(mrec),
                                        _ptr(match)), "ekf_sim_eval_match")
        return out, mrec, match

    def close(self):
        if getattr(self, "h", None) and self.h.value:
            lib().ekf_sim_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def lidar_config(**cfg) -> LidarConfig:
    """ekf_sim_lidar_config_default with fields set: its own, its ``scan``'s (lm_scan_config), or
    ``arena=(w, h)``."""
    c = LidarConfig()
    lib().ekf_sim_lidar_config_default(C.byref(c))
    if "arena" in cfg:
        c.scan.arena_w, c.scan.arena_h = cfg.pop("arena")
    own, scan = dict(LidarConfig._fields_), dict(ScanConfig._fields_)
    for name, v in cfg.items():
        if name in own and name != "scan":
            setattr(c, name, v)
        elif name in scan:
            setattr(c.scan, name, v)
        else:
            raise TypeError(f"unknown lidar setting {name!r}")
    return c


def eval_summary(recs) -> dict:
    """ekf_eval_summary of [F] records of EVAL_DTYPE (pure host code): a dict of ekf_eval_sum's
    fields."""
    recs = np.ascontiguousarray(recs, dtype=EVAL_DTYPE)
    out = EvalSum()
    _check(lib().ekf_eval_summary(_ptr(recs), len(recs), C.byref(out)), "ekf_eval_summary")
    return {name: getattr(out, name) for name, _ in EvalSum._fields_}


def poison_lds(device=0):
    """ekf_debug_poison_lds: every CU's LDS filled with a NaN pattern (tests: unwritten LDS reads
    then fail deterministically)."""
    _check(lib().ekf_debug_poison_lds(device), "ekf_debug_poison_lds")


def odometry(sc, track=None, radius=None):
    """t_odom_robot at each sensor message of a scenario, integrated natively by the product's
    DiffDrive::fkin (slam_integrate_odometry) — input preparation for ekf_replay."""
    track = sc.track if track is None else track
    radius = sc.radius if radius is None else radius
    wheel = _f64(sc.wheel)
    T, ticks = wheel.shape[0], wheel.shape[1]
    out = np.zeros((T, 3))
    _check(lib().slam_integrate_odometry(track, radius, T, ticks, _ptr(wheel), _ptr(out)),
           "slam_integrate_odometry")
    return out
