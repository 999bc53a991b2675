"""k_chain's lean wave-0 program as straight-line code: the sizes and positions it can get wrong.

The lean program's step is two basic blocks: its last step is peeled off the loop, the look-ahead
reads of the marker after next use a clamped index instead of a test, and every rare case of a
step (marker skipped or sighted for the first time, angles beyond normalize_angle_near's range, a
bad S) is folded into one word tested once, before the step's first store. Every test here runs a
drive twice on the HBM pipeline (EKF_RESIDENT=0), with EKF_CHAIN_FAST=1 and with EKF_CHAIN_FAST=0
(the generic program from step 0), and asks for the same bytes — state, Σ, t_map_odom, every
posterior pose — and for ekf_chain_path_counts to say where the lean program stopped:

* drives of tests/chain_cases.py and tests/edge_scenarios.py (N ≤ 130), lean + generic = corrections;
* messages of 1, 2, 3, 15 and 16 markers: the peeled step alone; no or one step with a marker
  after next; the clamped reads at the last columns of the block;
* a rare event at step 0, at a middle step and at the last step of a 16-marker chunk: a first
  sighting, an id out of range (skipped), and a heading that the step's own update throws beyond
  normalize_angle_near's range (the test found last, after K: see theta_case). The lean program
  ran exactly the markers before it;
* a handle created with EKF_CHAIN_FAST unset runs the lean program.

fp64 and fp32, simple and Joseph form. The helpers are tests/test_gpu_chain_fastpath.py's.
"""
import math

import numpy as np
import pytest

import chain_cases as cc
import orc
import pyekf
import test_gpu_chain_fastpath as fp

pytestmark = pytest.mark.gpu

FORMS, DTYPES = fp.FORMS, fp.DTYPES
POSITIONS = pytest.mark.parametrize("p", [0, 7, 15])
THETA_TARGET = 20.0   # rad; normalize_angle_near holds for |θ + π| < 5π = 15.7


def _both(monkeypatch, case, dtype, joseph):
    """→ the case's run with the lean program on, after checking it byte-equal to the run with the
    generic program alone and that program's counters."""
    fp._env(monkeypatch, "default", fast=True)
    pyekf.poison_lds()
    a = fp._run(case, dtype, joseph)
    fp._env(monkeypatch, "default", fast=False)
    b = fp._run(case, dtype, joseph)
    fp._same_bits(a, b)
    total = int(case.edge.count.sum())
    assert a["counts"].sum() == total
    assert b["counts"].sum(0).tolist() == [0, total]
    return a


@FORMS
@DTYPES
@pytest.mark.parametrize("name", ["clean_n130", "first_m20_p17", "two_p3_p9", "Z16_p15", "S_seam"])
def test_reused_drives(monkeypatch, name, dtype, joseph):
    case = cc.get(name)
    a = _both(monkeypatch, case, dtype, joseph)
    np.testing.assert_array_equal(a["counts"].sum(1), case.edge.count)
    want = cc.expected_counts(case, fp._ref(name, joseph)["events"])
    np.testing.assert_array_equal(a["counts"], want)


@FORMS
@DTYPES
@pytest.mark.parametrize("m", [1, 2, 3, 15, 16])
def test_chunk_sizes(monkeypatch, m, dtype, joseph):
    """Clean messages of m markers: every correction is the lean program's."""
    case = cc.populated(f"clean_cut{m}", 16, count=m)
    a = _both(monkeypatch, case, dtype, joseph)
    assert a["counts"].tolist() == [[m, 0]] * case.edge.n_messages
    assert not a["status"].any()


@FORMS
@DTYPES
@POSITIONS
def test_first_sighting_at(monkeypatch, p, dtype, joseph):
    case = cc.populated(f"first_at{p}", 16, withheld=((0, p),))
    a = _both(monkeypatch, case, dtype, joseph)
    assert a["counts"].tolist() == [[p, 16 - p]] + [[16, 0]] * (case.edge.n_messages - 1)


@FORMS
@DTYPES
@POSITIONS
def test_skipped_id_at(monkeypatch, p, dtype, joseph):
    """An id beyond the map at position p of message 0 (a device replay: the counters' totals)."""
    case = cc.populated(f"badid_at{p}", 16, bad=((0, p, 20 + 3),))
    assert case.how == "device"
    a = _both(monkeypatch, case, dtype, joseph)
    T = case.edge.n_messages
    assert a["counts"][-1].tolist() == [p + 16 * (T - 1), 16 - p]
    assert a["status"][-1] == pyekf.EKF_FLAG_RANGE


_theta: dict = {}


def theta_case(p):
    """The clean 16-marker drive with marker p of message 0 reported so far off in range that the
    correction's own update K·ν moves the heading to about THETA_TARGET: nothing about the marker is
    rare until the new heading fails normalize_angle_near, the last of the step's tests. The range
    offset comes from the oracle's state before that marker: the heading's gain row K[θ, :] by the
    filter's formulas (slam.cpp:219-261) in numpy, Δθ being linear in the innovation."""
    if p in _theta:
        return _theta[p]
    case = cc.populated(f"theta_at{p}", 16, n_msgs=1)
    e = case.edge
    x, S, tmo, cnt = case.start
    ref = orc.OracleEKF(n_landmarks=e.n_landmarks)
    ref.set(x, S, tmo, x[:3], cnt)
    ref.set_odom(e.odom[0])
    ref.predict()
    for i in range(p):
        assert ref.correct(int(e.ids[0, i]), *e.rel[0, i]) == 0
    x, S, _, _ = ref.get()
    lid, (rx, ry) = int(e.ids[0, p]), e.rel[0, p]
    k = 3 + 2 * lid
    idx = [0, 1, 2, k, k + 1]
    ex, ey = x[k] - x[1], x[k + 1] - x[2]
    d = ex * ex + ey * ey
    sd = math.sqrt(d)
    H = np.array([[0.0, -ex / sd, -ey / sd, ex / sd, ey / sd],
                  [-1.0, ey / d, -ex / d, -ey / d, ex / d]])
    Sm = H @ S[np.ix_(idx, idx)] @ H.T + 1e-2 * np.eye(2)   # (R: make_config's default)
    Kt = S[0, idx] @ H.T @ np.linalg.inv(Sm)
    z0 = math.hypot(rx, ry)
    nu = np.array([z0 - sd, orc.normalize_angle(math.atan2(ry, rx)
                                                - orc.normalize_angle(math.atan2(ey, ex) - x[0]))])
    base = x[0] + Kt @ nu
    b = (math.copysign(THETA_TARGET, Kt[0]) - base) / Kt[0]
    assert b > 0.0 and abs(base) < 1.0
    e.rel[0, p] *= (z0 + b) / z0
    _theta[p] = case
    return case


@FORMS
@DTYPES
@POSITIONS
def test_heading_thrown_out_at(monkeypatch, p, dtype, joseph):
    case = theta_case(p)
    a = _both(monkeypatch, case, dtype, joseph)
    print(a["counts"].tolist())
    assert a["counts"][0].tolist() == [p, 16 - p]
    np.testing.assert_array_equal(a["counts"].sum(1), case.edge.count)
    assert np.all(np.isfinite(a["x"])) and np.all(np.isfinite(a["S"]))


def test_default_is_lean(monkeypatch):
    """EKF_CHAIN_FAST unset at ekf_create: the lean program runs a clean drive's corrections."""
    case = cc.get("clean_m12")
    for k in fp.ENV_KEYS:
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("EKF_RESIDENT", "0")
    a = fp._run(case, pyekf.EKF_F64, False)
    assert a["counts"].sum(0).tolist() == [int(case.edge.count.sum()), 0]
