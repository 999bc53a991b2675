"""The C ABI of the marginals and the scoring (include/ekf.h ekf_get_marginals, ekf_eval,
ekf_eval_summary; include/ekf_sim.h ekf_sim_eval): declared, exported, bound, the records' layouts,
a NULL handle rejected with the outputs untouched, and ekf_eval_summary (pure host code) against
numpy — no GPU needed."""
import ctypes as C
import os
import re

import numpy as np

import pyekf

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY = {"ekf_get_marginals": "ekf.h", "ekf_eval": "ekf.h", "ekf_eval_summary": "ekf.h",
         "ekf_sim_eval": "ekf_sim.h"}
CHI2_3_95 = 7.814727903251179


def header(name):
    src = open(os.path.join(ROOT, "include", name)).read()
    return src, re.sub(r"/\*.*?\*/", "", src, flags=re.S)


def test_entry_points_declared_exported_and_listed():
    L = pyekf.lib()
    for name, h in ENTRY.items():
        assert re.search(r"^int\s+%s\s*\(" % name, header(h)[1], flags=re.M), (name, h)
        assert hasattr(L, name), name
        assert name in pyekf.EXPORTS, name
    # the binding's five entry points
    for obj, attr in ((pyekf.EKF, "marginals"), (pyekf.EKF, "eval"), (pyekf.Sim, "eval"),
                      (pyekf, "eval_summary")):
        assert callable(getattr(obj, attr))
    _, code = header("ekf.h")
    assert re.search(r"#define\s+EKF_EVAL_POSE_NOT_PD\s+1u", code)
    assert re.search(r"#define\s+EKF_EVAL_LM_NOT_PD\s+2u", code)
    assert (pyekf.EKF_EVAL_POSE_NOT_PD, pyekf.EKF_EVAL_LM_NOT_PD) == (1, 2)


def test_record_layouts():
    R, M = pyekf.EvalRec, pyekf.LmMarginal
    assert C.sizeof(R) == 128 and C.sizeof(M) == 48
    assert [(n, getattr(R, n).offset) for n, _ in R._fields_] == [
        ("pose_err", 0), ("pose_cov", 24), ("pose_nees", 72), ("lm_sq_err", 80), ("lm_nees", 88),
        ("lm_max_err", 96), ("lm_var_trace", 104), ("n_seen", 112), ("n_eval", 116),
        ("n_nees", 120), ("flags", 124)]
    assert [(n, getattr(M, n).offset) for n, _ in M._fields_] == [
        ("xy", 0), ("cov", 16), ("seen", 40), ("pad", 44)]
    # the numpy views of the same bytes
    assert pyekf.EVAL_DTYPE.itemsize == 128 and pyekf.LM_MARGINAL_DTYPE.itemsize == 48
    for n, _ in R._fields_:
        assert pyekf.EVAL_DTYPE.fields[n][1] == getattr(R, n).offset, n
    for n, _ in M._fields_:
        assert pyekf.LM_MARGINAL_DTYPE.fields[n][1] == getattr(M, n).offset, n
    # and the header's declarations, field by field in this order
    _, code = header("ekf.h")
    assert re.search(r"typedef struct \{\s*double xy\[2\];\s*double cov\[3\];\s*int seen;\s*"
                     r"int pad;\s*\} ekf_lm_marginal;", code)
    assert re.search(r"typedef struct \{\s*double pose_err\[3\];\s*double pose_cov\[6\];\s*"
                     r"double pose_nees, lm_sq_err, lm_nees, lm_max_err, lm_var_trace;\s*"
                     r"int n_seen, n_eval, n_nees;\s*unsigned flags;\s*\} ekf_eval_rec;", code)


def test_a_null_handle_is_rejected_and_nothing_is_written():
    L = pyekf.lib()
    pose, cov = np.full(3, 7.0), np.full(9, 7.0)
    lm = np.zeros(4, pyekf.LM_MARGINAL_DTYPE)
    lm["seen"] = 7
    cnt = np.full(1, 7, np.uint32)
    rc = L.ekf_get_marginals(None, 0, pose.ctypes.data, cov.ctypes.data, lm.ctypes.data,
                             cnt.ctypes.data)
    assert rc == pyekf.EKF_E_ARG
    assert (pose == 7).all() and (cov == 7).all() and (lm["seen"] == 7).all() and cnt[0] == 7
    out = np.zeros(2, pyekf.EVAL_DTYPE)
    out["n_seen"] = 7
    truth = np.zeros((2, 3))
    assert L.ekf_eval(None, truth.ctypes.data, None, 0, None, out.ctypes.data) == pyekf.EKF_E_ARG
    assert L.ekf_sim_eval(None, out.ctypes.data) == pyekf.EKF_E_ARG
    assert (out["n_seen"] == 7).all() and (out["pose_nees"] == 0).all()


def records(n, rng):
    r = np.zeros(n, pyekf.EVAL_DTYPE)
    r["pose_err"] = rng.normal(size=(n, 3)) * [0.02, 0.1, 0.1]
    r["pose_nees"] = rng.chisquare(3, n)
    r["n_eval"] = rng.integers(0, 9, n)
    r["n_nees"] = np.minimum(r["n_eval"], rng.integers(0, 9, n))
    r["n_seen"] = r["n_eval"] + 1
    r["lm_sq_err"] = rng.uniform(0, 1e-2, n) * r["n_eval"]
    r["lm_nees"] = rng.chisquare(2, n) * r["n_nees"]
    return r


def reference(r):
    ok = np.isfinite(r["pose_nees"])
    with np.errstate(invalid="ignore", divide="ignore"):
        return {
            "n": len(r), "n_pose_nees": int(ok.sum()),
            "anees_pose": r["pose_nees"][ok].sum() / ok.sum() if ok.any() else np.nan,
            "pose_in_95": (r["pose_nees"][ok] <= CHI2_3_95).sum() / ok.sum() if ok.any() else np.nan,
            "pos_rmse": np.sqrt((r["pose_err"][:, 1] ** 2 + r["pose_err"][:, 2] ** 2).mean()),
            "heading_rmse": np.sqrt((r["pose_err"][:, 0] ** 2).mean()),
            "lm_rmse": (np.sqrt(r["lm_sq_err"].sum() / r["n_eval"].sum())
                        if r["n_eval"].sum() else np.nan),
            "anees_lm": r["lm_nees"].sum() / r["n_nees"].sum() if r["n_nees"].sum() else np.nan,
        }


def same(got, ref, n):
    assert set(got) == set(ref)
    for k, v in ref.items():
        if isinstance(v, int):
            assert got[k] == v, k
        elif np.isnan(v):
            assert np.isnan(got[k]), k
        else:
            # sums of n non-negative terms in another order than numpy's pairwise one: n eps
            assert abs(got[k] - v) <= (n + 4) * 2.0 ** -52 * abs(v), (k, got[k], v)


def test_summary_against_numpy():
    rng = np.random.default_rng(5)
    r = records(37, rng)
    same(pyekf.eval_summary(r), reference(r), 37)
    # pose NEES that is NaN (a fresh filter) or infinite is left out of the mean and counted out
    r["pose_nees"][[3, 11, 30]] = np.nan
    r["pose_nees"][5] = np.inf
    got = pyekf.eval_summary(r)
    assert got["n"] == 37 and got["n_pose_nees"] == 33
    same(got, reference(r), 37)
    one = pyekf.eval_summary(r[:1])
    same(one, reference(r[:1]), 1)


def test_summary_ratios_with_a_zero_denominator_are_nan():
    rng = np.random.default_rng(6)
    r = records(5, rng)
    r["n_eval"] = 0
    r["n_nees"] = 0
    r["pose_nees"] = np.nan
    got = pyekf.eval_summary(r)
    assert got["n"] == 5 and got["n_pose_nees"] == 0
    for k in ("lm_rmse", "anees_lm", "anees_pose", "pose_in_95"):
        assert np.isnan(got[k]), k
    assert np.isfinite(got["pos_rmse"]) and np.isfinite(got["heading_rmse"])
    # landmarks evaluated, none with a positive definite block
    r["n_eval"] = 2
    r["lm_sq_err"] = 0.5
    got = pyekf.eval_summary(r)
    assert got["lm_rmse"] == np.sqrt(0.25) and np.isnan(got["anees_lm"])


def test_summary_share_within_the_95_percent_bound():
    r = np.zeros(4, pyekf.EVAL_DTYPE)
    r["pose_nees"] = [np.nextafter(CHI2_3_95, 0.0), CHI2_3_95, np.nextafter(CHI2_3_95, 10.0), 100.0]
    got = pyekf.eval_summary(r)
    assert got["n_pose_nees"] == 4 and got["pose_in_95"] == 0.5     # at or below the bound: in
    assert pyekf.eval_summary(r[:2])["pose_in_95"] == 1.0
    assert pyekf.eval_summary(r[2:])["pose_in_95"] == 0.0
    assert "7.814727903251179" in header("ekf.h")[0]


def test_summary_rejects_bad_arguments():
    L = pyekf.lib()
    r = np.zeros(2, pyekf.EVAL_DTYPE)
    out = pyekf.EvalSum()
    out.n = 7
    assert L.ekf_eval_summary(None, 2, C.byref(out)) == pyekf.EKF_E_ARG
    assert L.ekf_eval_summary(r.ctypes.data, 0, C.byref(out)) == pyekf.EKF_E_ARG
    assert L.ekf_eval_summary(r.ctypes.data, -1, C.byref(out)) == pyekf.EKF_E_ARG
    assert L.ekf_eval_summary(r.ctypes.data, 2, None) == pyekf.EKF_E_ARG
    assert out.n == 7
    assert L.ekf_eval_summary(r.ctypes.data, 2, C.byref(out)) == pyekf.EKF_OK and out.n == 2
