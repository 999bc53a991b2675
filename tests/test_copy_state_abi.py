"""The C ABI of the device-side state copy (include/ekf.h ekf_copy_state, include/ekf_sim.h
ekf_sim_fork): declared, exported, listed, bound, and a NULL handle or simulator rejected — no GPU
needed."""
import os
import re

import pyekf

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY = {"ekf_copy_state": ("ekf.h", r"ekf_t\s+dst,\s*int\s+dst_filter,\s*ekf_t\s+src,\s*"
                                     r"int\s+src_filter"),
         "ekf_sim_fork": ("ekf_sim.h", r"ekf_sim_t\s+dst,\s*ekf_sim_t\s+src,\s*int\s+src_filter")}


def header(name):
    src = open(os.path.join(ROOT, "include", name)).read()
    return re.sub(r"/\*.*?\*/", "", src, flags=re.S)


def test_entry_points_declared_exported_and_listed():
    L = pyekf.lib()
    for name, (h, args) in ENTRY.items():
        assert re.search(r"^int\s+%s\s*\(\s*%s\s*\)\s*;" % (name, args), header(h), flags=re.M), name
        assert hasattr(L, name), name
        assert name in pyekf.EXPORTS, name
        assert getattr(L, name).restype is pyekf.C.c_int
    assert callable(pyekf.EKF.copy_state_from) and callable(pyekf.Sim.fork_from)


def test_null_handles_are_rejected():
    L = pyekf.lib()
    for fd, fs in ((0, 0), (-1, 0), (-1, -1), (0, -1)):
        assert L.ekf_copy_state(None, fd, None, fs) == pyekf.EKF_E_ARG
    assert L.ekf_sim_fork(None, None, 0) == pyekf.EKF_E_ARG
