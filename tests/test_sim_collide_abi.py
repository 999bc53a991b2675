"""The C ABI of the simulator's collisions (include/ekf_sim.h ekf_sim_set_collisions,
ekf_sim_collisions, and the measurement hook ekf_sim_last_us): declared, exported, bound,
ekf_sim_config's layout untouched, and a NULL simulator and bad radii rejected — no GPU needed."""
import ctypes as C
import os
import re

import numpy as np

import pyekf

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY = {"ekf_sim_set_collisions": r"ekf_sim_t\s+s,\s*double\s+collision_radius,\s*double\s+"
                                   r"obstacle_radius",
         "ekf_sim_collisions": r"ekf_sim_t\s+s,\s*long long\s*\*\s*total,\s*int\s*\*\s*per_msg",
         "ekf_sim_last_us": r"ekf_sim_t\s+s,\s*double\s*\*\s*us"}


def header():
    src = open(os.path.join(ROOT, "include", "ekf_sim.h")).read()
    return re.sub(r"/\*.*?\*/", "", src, flags=re.S)


def test_entry_points_declared_exported_and_bound():
    L = pyekf.lib()
    for name, args in ENTRY.items():
        assert re.search(r"^int\s+%s\s*\(%s\);" % (name, args), header(), flags=re.M), name
        assert hasattr(L, name), name
        assert name in pyekf.EXPORTS and name in pyekf.LATER_EXPORTS, name
        assert name in pyekf.COLLIDE_EXPORTS + pyekf.SIM_DEV_EXPORTS
        assert getattr(L, name).argtypes is not None and getattr(L, name).restype is C.c_int
    assert L.ekf_sim_set_collisions.argtypes == [C.c_void_p, C.c_double, C.c_double]
    assert callable(pyekf.Sim.set_collisions) and callable(pyekf.Sim.collisions)
    assert callable(pyekf.Sim.last_us)
    # the measurement hook is kept apart from the feature's entry points
    assert pyekf.COLLIDE_EXPORTS == ("ekf_sim_set_collisions", "ekf_sim_collisions")
    assert pyekf.SIM_DEV_EXPORTS == ("ekf_sim_last_us",)


def test_the_configuration_is_as_it_was():
    """ekf_sim_config is mirrored by ctypes and by every caller: the collisions are set by a call,
    not by a field."""
    assert [n for n, _ in pyekf.SimConfig._fields_] == [
        "seed", "f0", "ticks_per_msg", "slip", "sensor_sigma", "max_range", "max_markers",
        "marker_stride", "wheel_radius", "track_width", "start_theta", "start_x", "start_y",
        "record"]
    assert C.sizeof(pyekf.SimConfig) == 96
    body = re.search(r"typedef struct \{(.*?)\} ekf_sim_config;", header(), flags=re.S).group(1)
    assert "collision" not in body and "obstacle" not in body


def test_null_simulator_and_bad_radii_are_rejected():
    L = pyekf.lib()
    total = np.full(2, 7, np.int64)
    per = np.full(4, 7, np.int32)
    assert L.ekf_sim_set_collisions(None, 0.11, 0.038) == pyekf.EKF_E_ARG
    for cr, orr in ((-0.11, 0.038), (0.11, -0.038), (math_nan(), 0.038), (0.11, math_nan()),
                    (-0.0 - 1e-300, 0.0)):
        assert L.ekf_sim_set_collisions(None, cr, orr) == pyekf.EKF_E_ARG
    assert L.ekf_sim_collisions(None, total.ctypes.data, per.ctypes.data) == pyekf.EKF_E_ARG
    assert L.ekf_sim_collisions(None, None, None) == pyekf.EKF_E_ARG
    assert (total == 7).all() and (per == 7).all()
    us = C.c_double(7.0)
    assert L.ekf_sim_last_us(None, C.byref(us)) == pyekf.EKF_E_ARG and us.value == 7.0


def math_nan():
    return float("nan")
