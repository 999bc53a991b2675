"""The pose trace's C ABI (include/ekf.h ekf_trace_*, include/slam_core.h slam_replay_trace):
declared, exported, bound, and rejecting a NULL handle — no GPU needed."""
import ctypes as C
import os
import re

import pyekf

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TRACE = {"ekf_trace_enable": "ekf.h", "ekf_trace_count": "ekf.h", "ekf_trace_read": "ekf.h",
         "ekf_trace_clear": "ekf.h", "slam_replay_trace": "slam_core.h"}


def test_trace_symbols_declared_exported_and_listed():
    L = pyekf.lib()
    for name, header in TRACE.items():
        src = open(os.path.join(ROOT, "include", header)).read()
        src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
        assert re.search(r"^int\s+%s\s*\(" % name, src, flags=re.M), (name, header)
        assert hasattr(L, name), name
        assert name in pyekf.EXPORTS, name


def test_trace_record_is_64_bytes():
    assert C.sizeof(pyekf.TraceRec) == 64
    assert pyekf.TraceRec.map_odom.offset == 24 and pyekf.TraceRec.seq.offset == 48
    src = open(os.path.join(ROOT, "include", "ekf.h")).read()
    assert re.search(r"typedef struct \{[^}]*double pose\[3\];[^}]*double map_odom\[3\];[^}]*"
                     r"long long seq;[^}]*long long reserved;[^}]*\} ekf_trace_rec;", src)


def test_trace_entry_points_reject_a_null_handle():
    L = pyekf.lib()
    n, got = C.c_longlong(7), C.c_int(7)
    rec = (pyekf.TraceRec * 2)()
    assert L.ekf_trace_enable(None, 8) == pyekf.EKF_E_ARG
    assert L.ekf_trace_count(None, 0, C.byref(n)) == pyekf.EKF_E_ARG
    assert L.ekf_trace_read(None, 0, 0, 2, C.addressof(rec), C.byref(got)) == pyekf.EKF_E_ARG
    assert L.ekf_trace_clear(None, -1) == pyekf.EKF_E_ARG
    w = (C.c_double * 2)()
    c = (C.c_int * 1)()
    assert L.slam_replay_trace(None, 1, 1, C.addressof(w), 0, C.addressof(c), None, None, None,
                               None, None) == pyekf.EKF_E_ARG
    assert (n.value, got.value) == (7, 7)  # outputs untouched
