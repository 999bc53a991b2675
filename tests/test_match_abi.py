"""The C ABI of the unknown-association run and its scoring (include/ekf.h ekf_eval_match;
include/ekf_sim.h ekf_sim_run_assoc, ekf_sim_eval_match): declared, exported, bound, the record's
layout, and a NULL handle rejected with the outputs untouched — no GPU needed."""
import ctypes as C
import os
import re

import numpy as np

import pyekf

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY = {"ekf_eval_match": "ekf.h", "ekf_sim_run_assoc": "ekf_sim.h",
         "ekf_sim_eval_match": "ekf_sim.h"}


def header(name):
    src = open(os.path.join(ROOT, "include", name)).read()
    return src, re.sub(r"/\*.*?\*/", "", src, flags=re.S)


def test_entry_points_declared_exported_and_bound():
    L = pyekf.lib()
    for name, h in ENTRY.items():
        assert re.search(r"^int\s+%s\s*\(" % name, header(h)[1], flags=re.M), (name, h)
        assert hasattr(L, name), name
        assert name in pyekf.EXPORTS, name
        assert getattr(L, name).argtypes is not None, name
    for obj, attr in ((pyekf.EKF, "eval_match"), (pyekf.Sim, "run_assoc"),
                      (pyekf.Sim, "eval_match")):
        assert callable(getattr(obj, attr))
    _, code = header("ekf.h")
    assert re.search(r"#define\s+EKF_MATCH_MAX_MAP\s+1024", code)
    assert pyekf.EKF_MATCH_MAX_MAP == 1024
    # the sentence that said so is gone
    assert "not supported here" not in header("ekf_sim.h")[0]


def test_record_layout():
    R = pyekf.MatchRec
    assert C.sizeof(R) == 32 and pyekf.MATCH_DTYPE.itemsize == 32
    assert [(n, getattr(R, n).offset) for n, _ in R._fields_] == [
        ("n_truth", 0), ("n_matched", 4), ("n_primary", 8), ("n_dup", 12), ("n_spurious", 16),
        ("n_missed", 20), ("max_match_dist", 24)]
    for n, _ in R._fields_:
        assert pyekf.MATCH_DTYPE.fields[n][1] == getattr(R, n).offset, n
    _, code = header("ekf.h")
    assert re.search(r"typedef struct \{\s*int n_truth;\s*int n_matched;\s*int n_primary;\s*"
                     r"int n_dup;\s*int n_spurious;\s*int n_missed;\s*double max_match_dist;\s*"
                     r"\} ekf_match_rec;", code)


def test_a_null_handle_is_rejected_and_nothing_is_written():
    L = pyekf.lib()
    out = np.zeros(2, pyekf.EVAL_DTYPE)
    out["n_seen"] = 7
    mrec = np.zeros(2, pyekf.MATCH_DTYPE)
    mrec["n_truth"] = 7
    match = np.full((2, 4), 7, np.int32)
    pose, lm = np.zeros((2, 3)), np.zeros((2, 4, 2))
    assert L.ekf_eval_match(None, pose.ctypes.data, lm.ctypes.data, 4, None, 0.5, out.ctypes.data,
                            mrec.ctypes.data, match.ctypes.data) == pyekf.EKF_E_ARG
    assert L.ekf_sim_eval_match(None, 0.5, out.ctypes.data, mrec.ctypes.data,
                                match.ctypes.data) == pyekf.EKF_E_ARG
    cmd = np.zeros((40, 2))
    assert L.ekf_sim_run_assoc(None, 1, cmd.ctypes.data) == pyekf.EKF_E_ARG
    assert L.ekf_sim_run_assoc(None, 0, None) == pyekf.EKF_E_ARG
    assert (out["n_seen"] == 7).all() and (mrec["n_truth"] == 7).all() and (match == 7).all()
