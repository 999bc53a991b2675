"""ekf_sim_run_lidar (include/ekf_sim.h): a Monte-Carlo run through the real sensor path whose data
never leaves the GPU — the simulator's truth poses, k_lidar_scan_swarm (lidar_kernels.hip) over them
and the simulator's maps, the landmark front-end's detect on its scans, and the association replay
of the handle's path over the detected markers and the simulator's odometry.

Twins, all exact. The scans: lm_simulate called per filter on the recorded truth poses with that
filter's cylinders, seed + f0 + f and scan0 = the run's first message — k_lidar_scan's bits, which
the culled kernel must reproduce for every input (its header comment has the argument), on maps of
both staging forms: below kCullFromMap cylinders a map is staged whole, from there on culled. The
posterior: a second handle fed through the host hop that the run removes (lm_simulate on host poses,
lm_detect_device on the scans uploaded again, lm_replay_into / lm_replay_resident with the host's
odometry) must end bit-identical in everything tests/test_gpu_sim_assoc.py::_same reads.

The host restatement synth.lidar_scans_counter is compared as tests/test_gpu_lidar_sim.py compares
it: within one float32 step away from grazing beams (that file's docstring has the reasoning)."""
import ctypes as C
import functools
import math
import os
import re

import numpy as np
import pytest

import landmarks_numpy as LN
import orc
import pyekf
from pyekf import synth
from pyekf.landmarks import Detector

import test_gpu_eval as tge
from test_gpu_lidar_sim import _grazing, _same_markers
from test_gpu_sim import _sim_for

pytestmark = pytest.mark.gpu

T = 12
MM = 32                       # detections kept per scan
R_OBS = 0.038
RANGE_MAX = 3.5
CULL = 2.0 ** -20             # lidar_kernels.hip kCullMargin
CULL_FROM = 32                # lm_launch.hpp kCullFromMap: smaller maps are staged whole
LID = dict(n_beams=360, max_markers=MM, threshold=0.2, obstacle_radius=R_OBS, seed=777,
           arena=(40.0, 40.0), range_max=RANGE_MAX, sigma=1e-3)


def _inc(B):
    return float(np.float32(2 * math.pi / B))


def _scan_kw(lid):
    """The lm_scan_config part of a run_lidar configuration, as Detector.simulate takes it."""
    return {k: lid[k] for k in ("arena", "range_max", "sigma") if k in lid}


def _circles(lm_f, r=R_OBS):
    return np.concatenate([lm_f, np.full((len(lm_f), 1), r)], 1)


def _culled(pose, circles, range_max=RANGE_MAX):
    """The kernel's own cull test on the host: which cylinders a scan from `pose` drops."""
    lx = pose[1] - 0.032 * math.cos(pose[0])
    ly = pose[2] - 0.032 * math.sin(pose[0])
    fx, fy = lx - circles[:, 0], ly - circles[:, 1]
    return np.sqrt(fx * fx + fy * fy) * (1.0 - CULL) - circles[:, 2] > range_max


def _twin_scans(det, truth, landmarks, lid, f0, msg0):
    """lm_simulate per filter on the recorded truth: [T, F, B] float32."""
    Tn, F = truth.shape[:2]
    out = np.zeros((Tn, F, lid["n_beams"]), np.float32)
    for f in range(F):
        out[:, f] = det.simulate(truth[:, f], _circles(landmarks[f], lid["obstacle_radius"]),
                                 n_beams=lid["n_beams"], seed=lid["seed"] + f0 + f, scan0=msg0,
                                 **_scan_kw(lid))
    return out


def _handle(N, F, dtype=pyekf.EKF_F64, joseph=False, trace=32):
    e = pyekf.EKF(n_landmarks=N, n_filters=F, dtype=dtype)
    if joseph:
        assert e.set_joseph(True) == 0
    if trace:
        e.trace_enable(trace)
    return e


def _same(a, b):
    ra, sa = tge._everything(a, MM)
    rb, sb = tge._everything(b, MM)
    assert ra == rb
    assert sa == sb
    return sa


def _close(*hs):
    for h in hs:
        h.close()


# ---- the scans: k_lidar_scan_swarm against lm_simulate -------------------------------------------

def _wide_map(F, L, half, seed):
    """L cylinders per filter, uniform in ±half, none within 0.4 m of the unit circle the robot
    drives (centre (0, 0) in the drive's frame: the path is |p − (0, 0)| = 1 around the start)."""
    rng = np.random.default_rng(seed)
    out = np.zeros((F, L, 2))
    for f in range(F):
        k = 0
        while k < L:
            p = rng.uniform(-half, half, 2)
            if abs(math.hypot(p[0], p[1]) - 1.0) >= 0.4:
                out[f, k] = p
                k += 1
    return out


@pytest.mark.parametrize("B", [360, 300])
def test_scans_equal_lm_simulate_per_filter(B):
    """F = 3, T = 5, L = 70 (two ballot rounds in wave 0, no multiple of 64), f0 = 5, two runs."""
    pyekf.poison_lds()
    N, F, Tn, L, f0 = 96, 3, 5, 70, 5
    sw = synth.swarm(N, F, 2 * Tn, survey=False, n_map=40)
    tpm = sw.wheel.shape[1]
    lm = _wide_map(F, L, 6.0, 11)
    e = _handle(N, F, trace=0)
    sim = pyekf.Sim(e, lm, seed=int(sw.seeds[0]), f0=f0, ticks_per_msg=tpm, max_markers=16,
                    marker_stride=16, start_theta=sw.start_pose[0], start_x=sw.start_pose[1],
                    start_y=sw.start_pose[2], record=1)
    det, det2 = (Detector(max_scans=Tn * F, max_beams=360) for _ in range(2))
    lid = dict(LID, n_beams=B)
    for run, msg0 in enumerate((0, Tn)):
        sim.run_lidar(det, sw.cmd[msg0 * tpm:(msg0 + Tn) * tpm], **lid)
        got = det.fetch_ranges()
        assert det.last_simulate_us() > 0.0
        _, truth = sim.poses()
        assert got.shape == (Tn * F, B) and got.dtype == np.float32
        # on the CPU: every scan drops some cylinders and keeps some
        for t in range(Tn):
            for f in range(F):
                n = int(_culled(truth[t, f], _circles(lm[f])).sum())
                assert 0 < n < L, (t, f, n)
        want = _twin_scans(det2, truth, lm, lid, f0, msg0)
        assert got.tobytes() == want.reshape(Tn * F, B).tobytes(), (run, B)
        # the scan headers lm_detect reads: a detect on the resident scans equals one on a copy
        cnt, mk = det.detect_resident(max_markers=MM)
        cnt2, mk2 = det2.detect(got, np.zeros(Tn * F), np.full(Tn * F, _inc(B)), max_markers=MM)
        _same_markers(cnt, mk, cnt2, mk2)
        # the host restatement, filter by filter
        for f in range(F):
            kw = dict(poses=truth[:, f], circles=_circles(lm[f]), n_beams=B)
            ref = synth.lidar_scans_counter(seed=lid["seed"] + f0 + f, scan0=msg0,
                                            arena=lid["arena"], sigma=lid["sigma"],
                                            range_max=RANGE_MAX, **kw)
            skip = _grazing(**kw)
            g = got.reshape(Tn, F, B)[:, f]
            step = np.abs(g.astype(np.float64) - ref.astype(np.float64)) / np.spacing(ref)
            print(f"run {run} B={B} f={f}: {skip.sum()} grazing, "
                  f"worst {step[~skip].max():.2f} steps")
            assert skip.sum() <= 0.005 * skip.size
            assert (step[~skip] <= 1.0).all()
            assert (ref < RANGE_MAX - 0.1).any()          # the scans see cylinders
    _close(sim, e, det, det2)


EDGE_SEED, EDGE_START = 20240317, (0.0, 0.0, -1.0)
EDGE_LID = dict(LID, sigma=0.0)


@functools.lru_cache(maxsize=None)
def _edge_pose():
    """The truth pose of the edge cases' only message (it does not depend on the map)."""
    sw = synth.swarm(50, 1, 1, survey=False, n_map=4, seed=EDGE_SEED)
    e = _handle(50, 1, trace=0)
    sim = _sim_for(e, sw)
    sim.run_assoc(sw.cmd)
    pose = sim.poses()[1][0, 0].copy()
    _close(sim, e)
    return sw.cmd.copy(), sw.wheel.shape[1], pose


def _ring(lidar, n, r0, r1, seed):
    rng = np.random.default_rng(seed)
    a, d = rng.uniform(0, 2 * math.pi, n), rng.uniform(r0, r1, n)
    return np.stack([lidar[0] + d * np.cos(a), lidar[1] + d * np.sin(a)], 1)


def _edge_maps(pose):
    th, x, y = pose
    lidar = (x - 0.032 * math.cos(th), y - 0.032 * math.sin(th))
    at = RANGE_MAX + R_OBS      # the centre distance at which the near face is at range_max
    beams = th + np.array([10, 80, 150, 220, 290]) * (2 * math.pi / 360)
    deltas = np.array([0.0, 1e-9, -1e-9, 1e-3, -1e-3])
    edge = np.stack([lidar[0] + (at + deltas) * np.cos(beams),
                     lidar[1] + (at + deltas) * np.sin(beams)], 1)
    # three more well inside, on beams of their own
    nb, nd = th + np.array([45, 115, 185]) * (2 * math.pi / 360), np.array([1.0, 1.5, 2.0])
    near = np.stack([lidar[0] + nd * np.cos(nb), lidar[1] + nd * np.sin(nb)], 1)
    # (the kernel culls maps of CULL_FROM cylinders and more: `boundary` is padded past that with
    # cylinders out of reach, and the two maps around the threshold mix reachable and not)
    far = _ring(lidar, CULL_FROM, 3.6, 9.0, 5)
    mixed = np.concatenate([_ring(lidar, 12, 0.5, 3.4, 6),
                            _ring(lidar, CULL_FROM - 12, 3.6, 9.0, 7)])
    return {
        # name: (map, cylinders that are out of reach)
        "boundary": (np.concatenate([edge, near, far]), 1 + CULL_FROM),
        "all_culled": (_ring(lidar, 70, 3.6, 9.0, 2), 70),
        "none_culled": (_ring(lidar, 70, 0.5, 3.4, 3), 0),
        "lds_full": (_ring(lidar, 1024, 0.5, 3.4, 4), 0),
        "below_threshold": (mixed[:-1], CULL_FROM - 13),
        "at_threshold": (mixed, CULL_FROM - 12),
    }


@pytest.mark.parametrize("name", ["boundary", "all_culled", "none_culled", "lds_full",
                                  "below_threshold", "at_threshold"])
def test_cull_edges_equal_lm_simulate(name):
    pyekf.poison_lds()
    launch_hpp = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                   "ekf-slam_amd", "csrc", "lm_launch.hpp")).read()
    assert int(re.search(r"kCullFromMap = (\d+);", launch_hpp).group(1)) == CULL_FROM
    cmd, tpm, pose = _edge_pose()
    lm, n_drop = _edge_maps(pose)[name]
    L = len(lm)
    assert (L >= CULL_FROM) == (name != "below_threshold")
    assert int(_culled(pose, _circles(lm)).sum()) == n_drop
    if name == "boundary":  # +1e-3 m is dropped; ±1e-9 m, 0 and −1e-3 m are inside the margin
        assert list(_culled(pose, _circles(lm))[:5]) == [False, False, False, True, False]
    N = max(50, L)
    e = _handle(N, 1, trace=0)
    sim = pyekf.Sim(e, lm, seed=EDGE_SEED, ticks_per_msg=tpm, max_markers=16, marker_stride=16,
                    start_theta=EDGE_START[0], start_x=EDGE_START[1], start_y=EDGE_START[2],
                    record=1)
    det, det2 = Detector(max_scans=1, max_beams=360), Detector(max_scans=1, max_beams=360)
    sim.run_lidar(det, cmd, **EDGE_LID)
    got = det.fetch_ranges()
    truth = sim.poses()[1]
    assert truth[0, 0].tobytes() == pose.tobytes()      # the map was laid out around this pose
    want = _twin_scans(det2, truth, lm[None], EDGE_LID, 0, 0)
    assert got.tobytes() == want.reshape(1, 360).tobytes()
    hit = got[0] < np.float32(RANGE_MAX)
    print(f"{name}: {int(hit.sum())} beams below range_max")
    assert hit.any() == (name != "all_culled")
    if name == "boundary":  # the cylinder 1e-3 m inside is seen; those at ±1e-9 m round to 3.5
        assert got[0, 290] < np.float32(RANGE_MAX) and got[0, 290] > np.float32(RANGE_MAX - 2e-3)
        assert (got[0, [10, 80, 150, 220]] == np.float32(RANGE_MAX)).all()
    _close(sim, e, det, det2)


# ---- end to end: the run against the host hop it removes ----------------------------------------

CASES = {  # N, F, n_map, dtype, joseph, path
    "pipeline96": (96, 2, 40, pyekf.EKF_F64, False, pyekf.EKF_PATH_PIPELINE),
    "resident50": (50, 3, 20, pyekf.EKF_F64, False, pyekf.EKF_PATH_RESIDENT),
    "f32-96": (96, 2, 40, pyekf.EKF_F32, False, pyekf.EKF_PATH_PIPELINE),
    "pipeline96-joseph": (96, 2, 40, pyekf.EKF_F64, True, pyekf.EKF_PATH_PIPELINE),
    "resident50-joseph": (50, 3, 20, pyekf.EKF_F64, True, pyekf.EKF_PATH_RESIDENT),
}


@functools.lru_cache(maxsize=None)
def _world(N, F, n_map):
    """The swarm, and on the CPU the preconditions of the end-to-end cases: on the host
    restatement's scans (synth's truth agrees with the device's to about 1e-14 m) at least half of
    the T·F scans publish a marker, and the oracle filter fed those markers raises nothing."""
    sw = synth.swarm(N, F, T + 4, survey=False, n_map=n_map)
    od = pyekf.odometry(sw.scenario(0))
    published = 0
    for f in range(F):
        scans = synth.lidar_scans_counter(sw.truth[:T, f], _circles(sw.landmarks[f]),
                                          seed=LID["seed"] + f, arena=LID["arena"],
                                          sigma=LID["sigma"], range_max=RANGE_MAX)
        ref = orc.OracleEKF(n_landmarks=N)
        for t in range(T):
            mk = LN.laser_callback(scans[t], 0.0, _inc(360))
            assert mk is not None and len(mk) <= MM
            ref.set_odom(od[t])
            if mk:
                published += 1
                rc, _, _ = ref.sensor_cb(np.array([[m[1], m[2]] for m in mk]))
                assert rc == 0, (f, t, rc)
    assert 2 * published >= T * F, published
    return sw


def _hop(e2, det2, sim, sw, msg0, lid=LID):
    """Today's route for the run `sim` just made: the truth poses to the host, lm_simulate filter by
    filter (each has its own seed), the scans uploaded again for lm_detect_device, and the replay
    with the odometry from the host."""
    odom, truth = sim.poses()
    Tn, F = truth.shape[:2]
    scans = _twin_scans(det2, truth, sw.landmarks, lid, 0, msg0)
    B = lid["n_beams"]
    det2.detect_device(scans.reshape(Tn * F, B), 0.0, _inc(B), lid["threshold"], MM)
    od = np.repeat(odom[:, None], F, 1)
    rc = (det2.replay_resident if e2.path == pyekf.EKF_PATH_RESIDENT else det2.replay_into)(
        e2, Tn, od)
    assert rc == pyekf.EKF_OK
    return scans


def _run_and_twin(name):
    N, F, n_map, dtype, joseph, path = CASES[name]
    sw = _world(N, F, n_map)
    tpm = sw.wheel.shape[1]
    e, e2 = _handle(N, F, dtype, joseph), _handle(N, F, dtype, joseph)
    assert e.path == path
    sim = _sim_for(e, sw)
    det, det2 = (Detector(max_scans=T * F, max_beams=360) for _ in range(2))
    sim.run_lidar(det, sw.cmd[:T * tpm], **LID)
    scans = _hop(e2, det2, sim, sw, 0)
    assert det.fetch_ranges().tobytes() == scans.tobytes()
    (cnt, mk), (cnt2, mk2) = det.fetch_markers(), det2.fetch_markers()
    _same_markers(cnt, mk, cnt2, mk2)
    assert 2 * int((cnt > 0).sum()) >= T * F
    status = _same(e, e2)
    assert status == [0] * F
    n_msgs = (cnt.reshape(T, F) > 0).sum(0)
    assert [e.trace_count(f) for f in range(F)] == list(n_msgs)
    print(name, "markers per scan:", cnt.reshape(T, F).T.tolist())
    _close(e2, det2)
    return sw, e, sim, det


@pytest.mark.parametrize("name", ["pipeline96", "resident50"])
def test_run_lidar_equals_the_host_hop(name):
    pyekf.poison_lds()
    N, F, n_map, dtype, joseph, _ = CASES[name]
    sw, e, sim, det = _run_and_twin(name)
    tpm = sw.wheel.shape[1]
    _, truth = sim.poses()

    # scoring: the slots matched to the simulator's map on the device
    start = np.array(sw.start_pose, np.float64)
    recs, mrecs, match = sim.eval_match(0.3)
    print(name, "match records:", mrecs)
    assert (mrecs["n_matched"] > 0).all()
    assert (mrecs["n_dup"] == mrecs["n_matched"] - mrecs["n_primary"]).all()
    assert (mrecs["n_missed"] == mrecs["n_truth"] - mrecs["n_primary"]).all()
    assert (mrecs["n_spurious"] == recs["n_seen"] - mrecs["n_matched"]).all()
    assert (mrecs["n_truth"] == n_map).all() and (recs["n_eval"] == mrecs["n_matched"]).all()
    want = e.eval_match(truth[-1], sw.landmarks, 0.3, frame=start)
    for a, b in zip((recs, mrecs, match), want):
        assert a.tobytes() == b.tobytes()

    # split: 7 + 5 messages end as the 12 did (and the scans of the second call as the tail)
    whole = det.fetch_ranges()
    es = _handle(N, F, dtype, joseph)
    sims = _sim_for(es, sw)
    dets = Detector(max_scans=T * F, max_beams=360)
    sims.run_lidar(dets, sw.cmd[:7 * tpm], **LID)
    assert dets.fetch_ranges().tobytes() == whole[:7 * F].tobytes()
    sims.run_lidar(dets, sw.cmd[7 * tpm:T * tpm], **LID)
    assert dets.fetch_ranges().tobytes() == whole[7 * F:].tobytes()
    _same(e, es)
    _close(sims, es, dets, sim, e, det)


@pytest.mark.parametrize("name", ["f32-96", "pipeline96-joseph", "resident50-joseph"])
def test_other_forms_equal_the_host_hop(name):
    pyekf.poison_lds()
    _, e, sim, det = _run_and_twin(name)
    _close(sim, e, det)


def test_run_lidar_alternates_with_run_assoc():
    """run_lidar, run_assoc, run_lidar on one simulator advance the counters run_assoc does: the
    poses (and the fake sensor's record) are those of a simulator that ran run_assoc three times,
    and the third run's scans are those of a twin at msg0 = 9."""
    pyekf.poison_lds()
    N, F, n_map = 96, 2, 40
    sw = _world(N, F, n_map)
    tpm = sw.wheel.shape[1]
    e, e0 = _handle(N, F), _handle(N, F, trace=0)
    sim, sim0 = _sim_for(e, sw), _sim_for(e0, sw)
    det, det2 = (Detector(max_scans=T * F, max_beams=360) for _ in range(2))
    for k, (a, b) in enumerate(((0, 4), (4, 9), (9, T))):
        cmd = sw.cmd[a * tpm:b * tpm]
        if k == 1:
            sim.run_assoc(cmd)
        else:
            sim.run_lidar(det, cmd, **LID)
        sim0.run_assoc(cmd)
        for x, y in zip(sim.poses() + sim.markers(), sim0.poses() + sim0.markers()):
            assert x.tobytes() == y.tobytes(), k
    want = _twin_scans(det2, sim.poses()[1], sw.landmarks, LID, 0, 9)
    assert det.fetch_ranges().tobytes() == want.reshape((T - 9) * F, 360).tobytes()
    _close(sim, sim0, e, e0, det, det2)


# ---- rejections ----------------------------------------------------------------------------------

def test_rejections(monkeypatch):
    pyekf.poison_lds()
    N, F, n_map = 96, 2, 40
    sw = _world(N, F, n_map)
    tpm = sw.wheel.shape[1]
    L = pyekf.lib()
    E = pyekf.EKF_E_ARG
    e = _handle(N, F)
    sim = _sim_for(e, sw)
    det = Detector(max_scans=2 * F, max_beams=360)
    cmd = np.ascontiguousarray(sw.cmd[:3 * tpm])
    # something resident and detected in the front-end, and a posterior in the filter, to be kept
    sim.run_lidar(det, cmd[:2 * tpm], **LID)
    before = tge._everything(e, MM)
    assert before[1] == [0] * F
    ranges, (cnt, mk) = det.fetch_ranges(), det.fetch_markers()

    def run(s=sim.h, d=det.h, Tn=2, c=cmd, **over):
        k = pyekf.lidar_config(**dict(LID, **over))
        return L.ekf_sim_run_lidar(s, d, Tn, None if c is None else c.ctypes.data, C.byref(k))

    nan = float("nan")
    assert run(s=None) == E and run(d=None) == E
    assert L.ekf_sim_run_lidar(sim.h, det.h, 2, cmd.ctypes.data, None) == E
    assert run(Tn=-1) == E and run(c=None) == E
    assert run(Tn=3) == E                                        # T·F > max_scans
    assert run(n_beams=1) == E and run(n_beams=361) == E
    assert run(max_markers=0) == E and run(max_markers=65) == E
    assert run(obstacle_radius=-1e-3) == E and run(obstacle_radius=nan) == E
    assert run(sigma=-1.0) == E and run(sigma=nan) == E
    assert run(range_min=4.0) == E and run(range_max=nan) == E   # range_min > range_max
    assert run(Tn=0, c=None, n_beams=1) == E                     # checked before T == 0 returns
    assert run(Tn=0, c=None) == pyekf.EKF_OK
    # the handle, the front-end's resident scans and markers, and the simulator's counters
    assert tge._everything(e, MM) == before
    assert det.fetch_ranges().tobytes() == ranges.tobytes()
    cnt1, mk1 = det.fetch_markers()
    assert cnt1.tobytes() == cnt.tobytes()
    _same_markers(cnt, mk, cnt1, mk1)
    e0 = _handle(N, F, trace=0)
    sim0 = _sim_for(e0, sw)
    sim0.run_assoc(cmd[:2 * tpm])
    sim0.run_assoc(cmd[2 * tpm:])
    sim.run_assoc(cmd[2 * tpm:])                                 # message 2 is the next one
    for x, y in zip(sim.poses() + sim.markers(), sim0.poses() + sim0.markers()):
        assert x.tobytes() == y.tobytes()
    _close(sim, sim0, e, e0, det)
    # a pipeline handle on the one-marker route has no device-planned association replay
    monkeypatch.setenv("EKF_ASSOC_MSG", "0")
    e = _handle(N, F)
    assert e.path == pyekf.EKF_PATH_PIPELINE and e.assoc_route == pyekf.EKF_ASSOC_MARKER
    sim = _sim_for(e, sw)
    det = Detector(max_scans=2 * F, max_beams=360)
    before = tge._everything(e, MM)
    assert run(s=sim.h, d=det.h) == E
    assert tge._everything(e, MM) == (before[0], [0] * F)
    out = np.zeros((2 * F, 360), np.float32)
    assert L.lm_fetch_ranges(det.h, out.ctypes.data) == E       # nothing became resident
    sim.run(cmd[:2 * tpm])                                       # the simulator has not moved
    assert (sim.markers()[0] == sw.count[:2]).all()
    _close(sim, e, det)
