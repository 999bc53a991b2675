"""The simulator's obstacle collisions on the device (ekf_sim_set_collisions, include/ekf_sim.h;
k_sim_collide and k_sim_pose_collide in ekf-slam_amd/csrc/sim_kernels.hip) on the cases of
tests/sim_collide_cases.py, which tests/test_sim_collide_cases.py pins on the CPU (each reaches its
path; no executed test d < R within GAP = 1e-6 of the other answer).

Per case:
* both forms on the pipeline, EKF_SIM_PARALLEL=0 (k_sim_collide) and =1 (k_sim_pose_collide): after
  every run the truth, odometry and marker positions against pyekf.synth within SIM_TOL = 1e-9,
  ids, actions and counts exactly (test_gpu_sim_edges' _check_inputs), the per-message and total
  collision counts exactly; the two forms' records are the same bytes;
* the candidate list's two forms, EKF_SIM_CULL_FROM=1 (always culled) and =2000 (the whole map,
  staged once): the same bytes again, so every case meets both whatever kCollideCullFromMap is;
* a drive cut into runs equals the same drive in one run, byte for byte;
* the filter: status 0; for N ≤ 128 both forms against the C oracle fed the device's recorded
  markers, at test_gpu_sim.py's bounds (5e-8 state, 1e-7 Σ: these maps too fold first sightings,
  the 1e7 prior, and corrections into one chunk); the parallel form also against a twin fed its
  recorded arrays (the same bytes). At N = 1024 the dense oracle takes minutes; there the
  sequential form's filter is held to the parallel one's, which that twin pins, at the bounds the
  suite already sets for one marker stream planned two ways (test_gpu_sim_edges' HOST_STATE_TOL =
  1e-9, HOST_SIGMA_TOL = 1e-8): the two forms hand the filter the same marker bytes (asserted), the
  sequential one through k_sim_collide's own descriptors, the parallel one through the device
  planner.
Cases with N ≤ 62 also run on the resident path (k_sim_collide again, from a resident handle).
"""
import math

import numpy as np
import pytest

import pyekf
from pyekf import synth
from pyekf.landmarks import Detector

import sim_collide_cases as cc
import test_gpu_sim_edges as edges

pytestmark = pytest.mark.gpu

R = cc.R
RESIDENT_CASES = ["head-on", "glance", "start-inside", "chain", "one-of-two"]


def _runs(sim, case, bounds=None):
    """Every run of the case: the inputs and the collision counts checked after each."""
    sw, tpm = case.sw, case.sw.wheel.shape[1]
    parts, hits = [], []
    for a, b in bounds or case.bounds:
        sim.run(sw.cmd[a * tpm:b * tpm], sw.sense[a:b])
        parts.append(edges._check_inputs(sim, sw, a))
        total, per_msg = sim.collisions()
        np.testing.assert_array_equal(per_msg, sw.hits[a:b])
        np.testing.assert_array_equal(total, sw.hits[:b].sum(0))
        hits.append(per_msg)
    return parts, hits


def _run_form(case, path, bounds=None, collide=True):
    e = pyekf.EKF(n_landmarks=case.n_slots, n_filters=case.sw.n_filters)
    assert e.path == path
    sim = pyekf.Sim(e, case.sw.landmarks, **case.sim_kw)
    if collide:
        sim.set_collisions(case.collision_radius, case.obstacle_radius)
    parts, hits = _runs(sim, case, bounds)
    got = edges._states(e)
    sim.close()
    e.close()
    return parts, got


def _truth_bytes(parts):
    return np.concatenate([p[5] for p in parts]).tobytes()


@pytest.mark.parametrize("name", cc.NAMES)
def test_case_on_the_pipeline_in_both_forms(name, monkeypatch):
    pyekf.poison_lds()
    case = cc.get(name)
    N = case.n_slots
    assert case.parallel
    monkeypatch.setenv("EKF_RESIDENT", "0")
    runs, states = {}, {}
    for env in ("0", "1"):
        print(f"{name}, EKF_SIM_PARALLEL={env}")
        monkeypatch.setenv("EKF_SIM_PARALLEL", env)
        parts, got = _run_form(case, pyekf.EKF_PATH_PIPELINE)
        runs[env] = parts
        if env == "1":   # the parallel form is ekf_replay_device over the recorded arrays
            e2 = edges._twin(case, N, parts, known=True)
            for (x, S, c), (x2, S2, c2) in zip(got, edges._states(e2)):
                assert x.tobytes() == x2.tobytes() and S.tobytes() == S2.tobytes() and c == c2
            e2.close()
        edges._against_oracle(case, N, parts, got)
        states[env] = got
    if N > edges.ORACLE_MAX_N:
        for (xa, Sa, ca), (xb, Sb, cb) in zip(states["0"], states["1"]):
            print(f"  sequential against parallel: state {np.abs(xa - xb).max():.3g}, sigma "
                  f"{np.abs(Sa - Sb).max():.3g}")
            assert ca == cb
            assert np.abs(xa - xb).max() < edges.HOST_STATE_TOL
            assert np.abs(Sa - Sb).max() < edges.HOST_SIGMA_TOL
    assert edges._bytes(runs["0"]) == edges._bytes(runs["1"])
    # the candidate list culled per message, and the whole map staged once
    for cull_from in ("1", "2000"):
        monkeypatch.setenv("EKF_SIM_CULL_FROM", cull_from)
        for env in ("0", "1"):
            monkeypatch.setenv("EKF_SIM_PARALLEL", env)
            parts, _ = _run_form(case, pyekf.EKF_PATH_PIPELINE)
            assert edges._bytes(parts) == edges._bytes(runs["0"]), (cull_from, env)
    monkeypatch.delenv("EKF_SIM_CULL_FROM")
    # one run equals the same drive split into several calls
    if len(case.bounds) > 1:
        T = case.sw.count.shape[0]
        for env in ("0", "1"):
            monkeypatch.setenv("EKF_SIM_PARALLEL", env)
            whole, _ = _run_form(case, pyekf.EKF_PATH_PIPELINE, bounds=((0, T),))
            assert _truth_bytes(whole) == _truth_bytes(runs["0"])
            for a, b in zip(edges._cat(whole), edges._cat(runs["0"])):
                assert a.tobytes() == b.tobytes()


@pytest.mark.parametrize("name", RESIDENT_CASES)
def test_case_on_the_resident_path(name):
    pyekf.poison_lds()
    case = cc.get(name)
    assert case.n_slots <= 62
    parts, got = _run_form(case, pyekf.EKF_PATH_RESIDENT)
    edges._against_oracle(case, case.n_slots, parts, got)


def test_head_on_is_held_while_odometry_goes_on():
    """The analytic result on the device: the final truth x is cx − R (1e-9 from the device's
    libm; the host restatement holds it to 1e-12), y and θ exactly 0, the odometry 0.8 m out."""
    case = cc.get("head-on")
    parts, _ = _run_form(case, pyekf.EKF_PATH_RESIDENT)
    odom, truth = parts[0][4], parts[0][5]
    cx = float(case.sw.landmarks[0, 0, 0])
    assert abs(truth[-1, 0, 1] - (cx - R)) < 1e-9 and truth[-1, 0, 2] == 0.0
    assert truth[-1, 0, 0] == 0.0 and abs(odom[-1, 1] - 0.8) < 1e-9


@pytest.mark.parametrize("form", ["parallel", "sequential", "resident"])
def test_nothing_in_reach_gives_the_bytes_of_collisions_off(form, monkeypatch):
    """Collisions on with no contact: truth, markers and filter state byte-equal to a second handle
    with collisions off (the optimistic message advances the truth by `wheels`' expression)."""
    pyekf.poison_lds()
    case = cc.get("clear" if form != "resident" else "one-of-two")
    if form == "resident":   # (N ≤ 62) filter 1 of one-of-two never collides: compare that one
        path = pyekf.EKF_PATH_RESIDENT
    else:
        path = pyekf.EKF_PATH_PIPELINE
        monkeypatch.setenv("EKF_RESIDENT", "0")
        monkeypatch.setenv("EKF_SIM_PARALLEL", "1" if form == "parallel" else "0")
    out = []
    for on in (True, False):
        e = pyekf.EKF(n_landmarks=case.n_slots, n_filters=case.sw.n_filters)
        assert e.path == path
        sim = pyekf.Sim(e, case.sw.landmarks, **case.sim_kw)
        if on:
            sim.set_collisions(case.collision_radius, case.obstacle_radius)
        sim.run(case.sw.cmd, case.sw.sense)
        total, per_msg = sim.collisions()
        rec = sim.markers() + sim.poses()
        out.append((rec, edges._states(e), total, per_msg))
        sim.close()
        e.close()
    (ra, sa, ta, pa), (rb, sb, tb, pb) = out
    assert not tb.any() and not pb.any()
    if form == "resident":
        assert ta[0] > 0 and ta[1] == 0
        f = 1
        for a, b in zip(ra[:4], rb[:4]):                    # counts, ids, actions, rel: [T, F, …]
            assert a[:, f].tobytes() == b[:, f].tobytes()
        assert ra[5][:, f].tobytes() == rb[5][:, f].tobytes()          # truth
        assert ra[4].tobytes() == rb[4].tobytes()                      # odometry (no collision's)
        assert ra[5][:, 0].tobytes() != rb[5][:, 0].tobytes()
        for a, b in zip(sa[f][:2], sb[f][:2]):
            assert a.tobytes() == b.tobytes()
    else:
        assert not ta.any() and not pa.any()
        for a, b in zip(ra, rb):
            assert a.tobytes() == b.tobytes()
        for (x, S, c), (x2, S2, c2) in zip(sa, sb):
            assert x.tobytes() == x2.tobytes() and S.tobytes() == S2.tobytes() and c == c2


def test_settings_rejections_and_turning_collisions_off():
    pyekf.poison_lds()
    case = cc.get("head-on")
    sw, tpm = case.sw, case.sw.wheel.shape[1]
    lib = pyekf.lib()
    free = synth._generate(case.n_slots, cc.straight(8), sw.seeds, sw.landmarks, start_pose=case.start,
                           slip=0.0)                            # the same drive, nothing in the way
    e = pyekf.EKF(n_landmarks=case.n_slots, n_filters=1)
    sim = pyekf.Sim(e, sw.landmarks, **case.sim_kw)
    sim.set_collisions(case.collision_radius, case.obstacle_radius)
    # refused, and the setting stays: the run below still collides
    for cr, orr in ((-1.0, 0.038), (0.11, -1.0), (math.nan, 0.038), (0.11, math.nan)):
        assert lib.ekf_sim_set_collisions(sim.h, cr, orr) == pyekf.EKF_E_ARG
    assert lib.ekf_sim_collisions(sim.h, None, None) == pyekf.EKF_E_ARG
    sim.run(sw.cmd[:5 * tpm])
    total, per_msg = sim.collisions()
    np.testing.assert_array_equal(per_msg, sw.hits[:5])
    assert np.abs(sim.poses()[1] - sw.truth[:5]).max() < 1e-9
    # off from the next run: the robot drives on into the cylinder from where it was held
    sim.set_collisions(0.0, case.obstacle_radius)
    sim.run(sw.cmd[5 * tpm:6 * tpm])
    total2, per_msg2 = sim.collisions()
    assert not per_msg2.any() and total2[0] == total[0] == sw.hits[:5].sum()
    truth = sim.poses()[1]
    step = free.truth[5, 0, 1] - free.truth[4, 0, 1]
    assert abs(truth[0, 0, 1] - (sw.truth[4, 0, 1] + step)).max() < 1e-9 and step > 0.09
    # on again, from inside the cylinder: pushed back out at once; the total goes on counting
    sim.set_collisions(case.collision_radius, case.obstacle_radius)
    sim.run(sw.cmd[6 * tpm:])
    total3, per_msg3 = sim.collisions()
    assert per_msg3[:, 0].tolist() == [tpm, tpm] and total3[0] == total[0] + 2 * tpm
    assert np.abs(sim.poses()[1][:, 0] - sw.truth[6:, 0]).max() < 1e-9
    sim.close()
    # without cfg.record there is no per-message count, and the totals still come
    sim = pyekf.Sim(e, sw.landmarks, **{**case.sim_kw, "record": 0})
    sim.set_collisions(case.collision_radius, case.obstacle_radius)
    sim.run(sw.cmd[:5 * tpm])
    tot = np.zeros(1, np.int64)
    per = np.zeros((5, 1), np.int32)
    assert lib.ekf_sim_collisions(sim.h, tot.ctypes.data, per.ctypes.data) == pyekf.EKF_E_ARG
    assert sim.collisions(per_msg=False)[0][0] == sw.hits[:5].sum()
    sim.close()
    e.close()


# ---- unknown association and the laser, on a drive that would cross cylinders --------------------
N_X, F_X, T_X = 96, 2, 8


def _crossing():
    """The unit circle of synth.swarm (start (0, −1) heading +x, 0.1 rad a message) with two
    cylinders in the way: 0.3 rad along at radius 1.08 and 0.6 rad along at radius 0.92."""
    sw = synth.swarm(N_X, F_X, T_X, survey=False, n_map=40)
    lm = sw.landmarks.copy()
    for i, (ang, rad) in enumerate(((0.3, 1.08), (0.6, 0.92))):
        lm[:, i] = (rad * math.sin(ang), -rad * math.cos(ang))
    return sw, lm


def _sim(e, sw, lm, collide):
    sim = pyekf.Sim(e, lm, seed=int(sw.seeds[0]), ticks_per_msg=sw.wheel.shape[1], max_markers=16,
                    marker_stride=16, start_theta=sw.start_pose[0], start_x=sw.start_pose[1],
                    start_y=sw.start_pose[2], record=1)
    if collide:
        sim.set_collisions(cc.COLLISION_RADIUS, cc.OBSTACLE_RADIUS)
    return sim


def _clearance(truth, lm):
    """[T, F] distance from the body centre to the nearest cylinder centre, and from the lidar."""
    d = np.hypot(lm[None, :, :, 0] - truth[:, :, None, 1], lm[None, :, :, 1] - truth[:, :, None, 2])
    lx = truth[..., 1] - 0.032 * np.cos(truth[..., 0])
    ly = truth[..., 2] - 0.032 * np.sin(truth[..., 0])
    dl = np.hypot(lm[None, :, :, 0] - lx[..., None], lm[None, :, :, 1] - ly[..., None])
    return d.min(2), dl.min(2)


def test_run_assoc_and_run_lidar_with_collisions_on():
    pyekf.poison_lds()
    sw, lm = _crossing()
    out = {}
    for kind in ("off", "assoc", "lidar"):
        e = pyekf.EKF(n_landmarks=N_X, n_filters=F_X)
        assert e.path == pyekf.EKF_PATH_PIPELINE
        sim = _sim(e, sw, lm, kind != "off")
        det = None
        if kind == "lidar":
            det = Detector(max_scans=T_X * F_X, max_beams=360)
            sim.run_lidar(det, sw.cmd, n_beams=360, max_markers=32, threshold=0.2,
                          obstacle_radius=cc.OBSTACLE_RADIUS, seed=777, arena=(40.0, 40.0),
                          range_max=3.5, sigma=0.0)
            out["ranges"] = det.fetch_ranges().reshape(T_X, F_X, 360)
        else:
            sim.run_assoc(sw.cmd)
        total, per_msg = sim.collisions()
        _, truth = sim.poses()
        assert [e.status(f) for f in range(F_X)] == [0] * F_X
        if kind == "assoc":   # the run is scored on the device as without collisions
            recs, mrecs, match = sim.eval_match(0.3)
            print("match records:", mrecs)
            assert (mrecs["n_matched"] > 0).all() and (mrecs["n_truth"] == 40).all()
            assert (mrecs["n_missed"] == mrecs["n_truth"] - mrecs["n_primary"]).all()
            assert np.isfinite(recs["pose_err"]).all()
        out[kind] = (truth, total, per_msg)
        for h in (sim, e, det):
            if h is not None:
                h.close()
    body_off, _ = _clearance(out["off"][0], lm)
    body, lidar = _clearance(out["assoc"][0], lm)
    print("nearest centre, off:", body_off.min(0), "on:", body.min(0), "lidar:", lidar.min(0),
          "hits:", out["assoc"][1], "min range:", out["ranges"].min())
    # without collisions the drive goes well inside a cylinder's reach; with them it is kept out of every one
    assert (body_off.min(0) < R - 0.05).all() and not out["off"][1].any()
    assert (out["assoc"][1] > 0).all() and out["assoc"][2].sum(0).tolist() == out["assoc"][1].tolist()
    # what the rule guarantees with cylinders that do not overlap: the body centre at R or more from
    # every centre, so the lidar, 0.032 m behind it, at R − 0.032 or more, 0.078 m off the surface
    assert (body >= R - 1e-9).all() and (lidar >= R - 0.032 - 1e-9).all()
    # the lidar run: the same truth and counts as the association run's twin. The range bound is the
    # issue's: no beam shorter than the robot's own collision radius. The rule alone gives only the
    # 0.078 m above; it holds here because this geometry keeps the lidar further off at the sampled
    # poses (printed) and because range_min, 0.11 by default, clamps a scan from below anyway
    assert out["lidar"][0].tobytes() == out["assoc"][0].tobytes()
    np.testing.assert_array_equal(out["lidar"][1], out["assoc"][1])
    np.testing.assert_array_equal(out["lidar"][2], out["assoc"][2])
    assert (out["ranges"].min(2) >= cc.COLLISION_RADIUS - 1e-9).all()
    assert (out["ranges"].min(2) < 3.5).all()                       # the scans see cylinders
