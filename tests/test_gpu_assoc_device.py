"""ekf_replay_device_assoc (include/ekf.h): an unknown-association replay (Slam::sensor_cb,
nuslam/src/slam.cpp:318-530, per message) whose inputs already live on the GPU, its chunk
descriptors planned by k_plan_assoc (plan_kernels.hip); ekf_get_decisions; and the front-end's
device-side hand-off lm_detect_device → lm_replay_into (include/landmarks.h). Parity: the same
messages through the host planner (ekf_replay with assoc = 1, Planner::unknown in ekf_plan.cpp) and
the CPU oracles (OracleEKF.sensor_cb, landmarks_numpy.laser_callback).

fp64 N = 96 (n = 195: the HBM pipeline, two workgroups of k_assoc_msg per filter, so the exchange
runs) unless stated. Tolerances, device- against host-planned: the project's own for such replays
(tests/test_gpu_replay_device.py): state 1e-9, Σ 1e-8, counters and status words exact. The two
plans differ only in the last bit of a bearing, and only where glibc's atan2 on the host is not the
correctly rounded value the device computes (atan2_dd.hpp; about one marker in a thousand): most
cases below end bit-identical, the largest difference measured is 1.5e-11 on the state and 1.9e-9
on Σ. (With ocml's atan2 on the device the 30-message case ended 3.2e-9 apart on the state: the
prior's 1e7 − (1e7 − δ) turns every differing bit into another rounding of a new landmark's Σ.)

A last-bit change of a bearing can flip a decision only where it sits on the gate or ties with the
runner-up. Every drive below is therefore first run through the oracle alone, marker by marker,
and the Mahalanobis distances (slam.cpp:353-399) of each marker to every mapped landmark are
computed with numpy from the oracle's state and Σ: the smallest one must differ from mah_gate by
more than 1e-6 relative, and the best and second-best candidates (the forced new slot at the gate
among them, slam.cpp:401-408) by more than 1e-6 relative. The seeds are chosen so that this holds."""
import ctypes as C
import functools
import math
import os

import numpy as np
import pytest

import landmarks_numpy as L
import orc
import pyekf
from pyekf import synth

pytestmark = pytest.mark.gpu

N = 96
GATE, R_NOISE = 2.0, 1e-2
MARGIN = 1e-6
STATE_TOL, SIGMA_TOL = 1e-9, 1e-8   # tests/test_gpu_replay_device.py:14-18
ENV = ("EKF_SERIAL", "EKF_CU_SPLIT", "EKF_DEVSYNC", "EKF_AM_XCD", "EKF_ASSOC_MSG", "EKF_STAGE",
       "EKF_RESIDENT")
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "scans.npz")
BASIC = [(-0.5, -0.7, 0.038), (0.8, -0.8, 0.038), (0.4, 0.8, 0.038), (-0.6, 0.65, 0.038)]


def _env(monkeypatch, **kv):
    for k in ENV:
        monkeypatch.delenv(k, raising=False)
    for k, v in kv.items():
        monkeypatch.setenv(k, v)


# ---- the oracle alone: decisions, poses and the margins of every decision ----

def _distances(x, S, counter, z):
    """Squared Mahalanobis distance of measurement z = (range, bearing) to landmarks 0..counter−1
    (slam.cpp:353-399) from the oracle's state x and covariance S."""
    if counter == 0:
        return np.zeros(0)
    j = 3 + 2 * np.arange(counter)
    dx, dy = x[j] - x[1], x[j + 1] - x[2]
    d = dx * dx + dy * dy
    rt = np.sqrt(d)
    H = np.zeros((counter, 2, 5))
    H[:, 0, 1], H[:, 0, 2], H[:, 0, 3], H[:, 0, 4] = -dx / rt, -dy / rt, dx / rt, dy / rt
    H[:, 1, 0], H[:, 1, 1], H[:, 1, 2], H[:, 1, 3], H[:, 1, 4] = -1.0, dy / d, -dx / d, -dy / d, dx / d
    idx = np.stack([0 * j, 0 * j + 1, 0 * j + 2, j, j + 1], 1)
    P = S[idx[:, :, None], idx[:, None, :]]
    psi = H @ P @ H.transpose(0, 2, 1) + R_NOISE * np.eye(2)
    db = z[1] - (np.arctan2(dy, dx) - x[0])
    dz = np.stack([z[0] - rt, (db + math.pi) % (2 * math.pi) - math.pi], 1)
    return np.einsum("ki,ki->k", dz, np.linalg.solve(psi, dz[..., None])[..., 0])


def _oracle_message(ref, rel, check=True):
    """sensor_cb marker by marker (as OracleEKF.sensor_cb_dmin runs it), asserting the margins of
    every decision first. Returns (assoc, is_new)."""
    lib = orc.lib()
    m = len(rel)
    j, nw = np.zeros(m, np.int32), np.zeros(m, np.int32)
    if m == 0:
        return j, nw
    lib.orc_ekf_predict(ref.h)
    for i in range(m):
        if check:
            x, S, _, c = ref.get()
            z = (math.sqrt(rel[i, 0] ** 2 + rel[i, 1] ** 2), math.atan2(rel[i, 1], rel[i, 0]))
            d = _distances(x, S, c, z)
            if d.size:
                assert abs(d.min() - GATE) > MARGIN * GATE, (i, d.min())
                cand = np.sort(np.append(d, GATE))  # the forced new slot sits at the gate
                assert cand[1] - cand[0] > MARGIN * cand[1], (i, cand[:2])
        jj, nn = C.c_int(-1), C.c_int(0)
        rc = lib.orc_ekf_associate_correct(ref.h, float(rel[i, 0]), float(rel[i, 1]),
                                           C.byref(jj), C.byref(nn))
        assert rc == 0
        j[i], nw[i] = jj.value, nn.value
    lib.orc_ekf_posterior(ref.h)
    return j, nw


def _oracle_drive(cnt, rel, od, joseph=False, check_from=0, ref=None):
    """One filter's messages (cnt[t] <= 0: none) through the oracle; the margins are asserted from
    message check_from on. Returns (ref, decisions per message, pose after each message)."""
    ref = ref or orc.OracleEKF(n_landmarks=N, mah_gate=GATE, joseph=joseph)
    dec, poses = [], []
    for t in range(len(cnt)):
        ref.set_odom(od[t])
        c = max(int(cnt[t]), 0)
        dec.append(_oracle_message(ref, rel[t, :c], check=t >= check_from))
        poses.append(ref.get(sigma=False)[0][:3].copy())
    return ref, dec, np.array(poses)


@functools.lru_cache(maxsize=None)
def _case(F, T, M, seed, holes, joseph=False, check_from=0):
    """F robots × T messages of at most M markers (robot f: synth.synthetic seed + f, shuffled).
    holes: filter 1 gets no message on some steps (count 0 or −1), and one full message of
    filter 0 reports more markers than M (the front-end counts what it could not write).
    Returns cnt_dev, cnt_host (clamped to [0, M]), rel, odom and the oracle's run per filter."""
    cnt = np.zeros((T, F), np.int32)
    rel = np.zeros((T, F, M, 2))
    od = np.zeros((T, F, 3))
    scs = []
    for f in range(F):
        sc = synth.synthetic(N, T, seed=seed + f, max_markers=M, shuffle=True)
        scs.append(sc)
        cnt[:, f] = sc.count
        if M > 17:  # messages of 17 to M markers: two and three chunks, in turn
            cnt[:, f] = np.minimum(sc.count, np.roll([M, 17, 33, 25], f)[np.arange(T) % 4])
        rel[:, f] = sc.rel
        od[:, f] = pyekf.odometry(sc)
    dev = cnt.copy()
    if holes:
        if F > 1:
            dev[1::3, 1] = 0
            dev[2::6, 1] = -1
        full = np.flatnonzero(cnt[:, 0] == M)
        assert full.size
        dev[full[full.size // 2], 0] = M + 5
    host = np.clip(dev, 0, M).astype(np.int32)
    for a in (dev, host, rel, od):
        a.setflags(write=False)
    oracle = [_oracle_drive(host[:, f], rel[:, f], od[:, f], joseph, check_from) for f in range(F)]
    return dev, host, rel, od, oracle, scs


# ---- the GPU runs ----

def _gpu(arrs):
    import torch
    return tuple(torch.from_numpy(np.array(a, order="C")).cuda() for a in arrs)


def _read(e):
    return ([e.state(f) for f in range(e.F)], [e.status(f) for f in range(e.F)],
            np.stack([e.pose(f) for f in range(e.F)]))


def _run(kind, F, cnt, rel, od, dtype=pyekf.EKF_F64, joseph=False, warm=None):
    e = pyekf.EKF(n_landmarks=N, n_filters=F, dtype=dtype)
    assert e.path == pyekf.EKF_PATH_PIPELINE
    if joseph:
        assert e.set_joseph(True) == pyekf.EKF_OK
    assert e.assoc_route != pyekf.EKF_ASSOC_MARKER
    if warm is not None:
        x, S, tmo, c = warm
        for f in range(F):
            e.set_state(x, S, tmo=tmo, counter=c, f=f)
    if kind == "device":
        g = _gpu((cnt, rel, od))
        e.replay_device_assoc(*g)
    else:
        e.replay(np.clip(cnt, 0, rel.shape[2]), rel, od, assoc=True)
    out = _read(e)
    e.close()
    return out


def _close(a, b, tol=STATE_TOL, stol=SIGMA_TOL):
    (sa, fa, pa), (sb, fb, pb) = a, b
    print("device- against host-planned, per filter (state, sigma):",
          [(float(np.abs(xa - xb).max()), float(np.abs(Sa - Sb).max()))
           for (xa, Sa, _), (xb, Sb, _) in zip(sa, sb)])
    assert fa == fb
    for (xa, Sa, ca), (xb, Sb, cb) in zip(sa, sb):
        assert ca == cb
        assert np.abs(xa - xb).max() <= tol
        assert np.abs(Sa - Sb).max() <= stol
    assert np.abs(pa - pb).max() <= tol


def _compare(F, T, M, seed, holes=True, joseph=False):
    dev, host, rel, od, oracle, _ = _case(F, T, M, seed, holes, joseph)
    d = _run("device", F, dev, rel, od, joseph=joseph)
    h = _run("host", F, host, rel, od, joseph=joseph)
    assert d[1] == [0] * F
    _close(d, h)
    for f in range(F):  # ... and where the oracle ends (counter exact)
        assert d[0][f][2] == oracle[f][0].get(sigma=False)[3] > 0
    return d, oracle


# ---- 1–3: equal to the host plan ----

@pytest.mark.parametrize("F,env", [(1, {}), (3, {}), (1, {"EKF_SERIAL": "1"}),
                                   (1, {"EKF_DEVSYNC": "0"}), (1, {"EKF_AM_XCD": "0"})],
                         ids=["1filter", "3filters", "1filter_serial", "1filter_events",
                              "1filter_agent"])
def test_device_assoc_replay_equals_host_replay(monkeypatch, F, env):
    """30 messages of up to 16 markers, packed pairs (stride 2), every schedule and both exchange
    placements: the device-planned replay ends where the host-planned one does. Filter 1 sits
    messages out (count 0 and −1), one message reports more markers than m_max (clamped)."""
    _env(monkeypatch, **env)
    pyekf.poison_lds()
    _compare(F, 30, 16, 7)


@pytest.mark.parametrize("M", [17, 40])
def test_device_assoc_replay_several_chunks(monkeypatch, M):
    """m_max = 17 and 40: two and three chunk launches a message (16 + 1 markers; up to 16 + 16 +
    8), every chunk's decisions at its own assoc_slot, kFirst / kLast on different chunks."""
    _env(monkeypatch)
    pyekf.poison_lds()
    dev, host, *_ = _case(2, 12, M, 23, True)
    assert host.max() == M and (host[host > 0] >= 17).all()
    _compare(2, 12, M, 23)


def test_device_assoc_replay_70_messages(monkeypatch):
    """T = 70 in one call: the planner's parity scan takes a second round of 64 messages."""
    _env(monkeypatch)
    pyekf.poison_lds()
    _compare(2, 70, 16, 31)


# ---- 4: decisions ----

def test_decisions_equal_oracle_and_single_call_is_bit_identical(monkeypatch):
    """One call per message (T = 1) and ekf_get_decisions behind each: every decision equals the
    oracle's sensor_cb, every posterior pose is within 1e-8 (tests/test_gpu_pipeline.py). The same
    drive in one call ends bit-identical: the mirror exported per call and the one chained on the
    device plan the same descriptors."""
    _env(monkeypatch)
    pyekf.poison_lds()
    T, M = 20, 16
    dev, host, rel, od, oracle, _ = _case(1, T, M, 41, False)
    _, dec, poses = oracle[0]
    e = pyekf.EKF(n_landmarks=N)
    keep, n_new, n_old = [], 0, 0
    for t in range(T):
        g = _gpu((dev[t:t + 1], rel[t:t + 1], od[t:t + 1]))
        keep.append(g)
        e.replay_device_assoc(*g)
        c = int(host[t, 0])
        j, nw = e.decisions(c)
        np.testing.assert_array_equal(j, dec[t][0])
        np.testing.assert_array_equal(nw, dec[t][1])
        n_new += int(nw.sum())
        n_old += int(c - nw.sum())
        assert np.abs(e.pose() - poses[t]).max() < 1e-8, t
    assert n_new > 0 and n_old > 0
    per = _read(e)
    e.close()
    one = _run("device", 1, dev, rel, od)
    assert per[1] == one[1] == [0]
    assert per[0][0][2] == one[0][0][2]
    np.testing.assert_array_equal(per[0][0][0], one[0][0][0])
    np.testing.assert_array_equal(per[0][0][1], one[0][0][1])
    # ekf_get_decisions after a host-planned message too (ekf_sensor without outputs)
    e = pyekf.EKF(n_landmarks=N)
    e.set_odom(od[0, 0])
    assert e.sensor(rel[0, 0, :int(host[0, 0])], decisions=False)[0] == pyekf.EKF_OK
    j, nw = e.decisions(int(host[0, 0]))
    np.testing.assert_array_equal(j, dec[0][0])
    np.testing.assert_array_equal(nw, dec[0][1])
    e.close()


# ---- 5: both dtypes and forms ----

def test_device_assoc_replay_fp32(monkeypatch):
    """fp32 Σ from an fp64 association warm-up of 20 messages, then 12 messages device- against
    host-planned at the host-against-device figures of test_device_replay_fp32_n1024 (1e-6)."""
    _env(monkeypatch)
    pyekf.poison_lds()
    W, T, M = 20, 32, 16
    dev, host, rel, od, oracle, _ = _case(1, T, M, 53, False)
    e = pyekf.EKF(n_landmarks=N)
    e.replay(host[:W], rel[:W], od[:W], assoc=True)
    x, S, c = e.state()
    ws = (x, S, e.map_odom(), c)
    assert e.status() == 0 and c > 0
    e.close()
    d = _run("device", 1, dev[W:], rel[W:], od[W:], dtype=pyekf.EKF_F32, warm=ws)
    h = _run("host", 1, host[W:], rel[W:], od[W:], dtype=pyekf.EKF_F32, warm=ws)
    assert d[1] == [0]
    assert np.all(np.isfinite(d[0][0][1]))
    assert d[0][0][2] == oracle[0][0].get(sigma=False)[3]
    _close(d, h, 1e-6, 1e-6)


def test_device_assoc_replay_joseph(monkeypatch):
    """The Joseph form (ekf_set_joseph: every chunk flagged kJoseph, k_assoc_msg<T, true>), fp64,
    at the tolerances of the simple form."""
    _env(monkeypatch)
    pyekf.poison_lds()
    _compare(2, 20, 16, 61, joseph=True)


# ---- 6: hand-over ----

def test_handover_known_host_assoc_device_known_device(monkeypatch):
    """A known-id ekf_replay, the device association replay, a known-id ekf_replay_device, then a
    state read — against the same spans all planned on the host. The drive's first 64 messages
    (a whole revolution: every landmark in view is mapped) go through the oracle; the filters start
    from its state, and the known-id spans carry the oracle's own decisions as their ids."""
    _env(monkeypatch)
    pyekf.poison_lds()
    W, T, M = 64, 94, 16
    spans = [(64, 72), (72, 84), (84, 94)]
    dev, host, rel, od, oracle, _ = _case(1, T, M, 72, False, False, spans[1][0])
    _, dec, _ = oracle[0]
    ids = np.zeros((T, 1, M), np.int32)
    for t in range(T):
        ids[t, 0, :len(dec[t][0])] = dec[t][0]
    assert not any(dec[t][1].any() for t in range(W, T))  # the map is complete: no new landmark
    ref, _, _ = _oracle_drive(host[:W, 0], rel[:W, 0], od[:W, 0], check_from=W)
    x, S, tmo, c = ref.get()
    act = np.zeros_like(ids)
    res = []
    for kinds in (("host", "device", "device"), ("host", "host", "host")):
        e = pyekf.EKF(n_landmarks=N)
        e.set_state(x, S, tmo=tmo, counter=c)
        keep = []
        for i, ((t0, t1), kind) in enumerate(zip(spans, kinds)):
            sl = slice(t0, t1)
            if kind == "host":
                e.replay(host[sl], rel[sl], od[sl], ids=ids[sl] if i != 1 else None,
                         actions=act[sl] if i != 1 else None, assoc=i == 1)
            elif i == 1:
                keep.append(_gpu((dev[sl], rel[sl], od[sl])))
                e.replay_device_assoc(*keep[-1])
            else:
                keep.append(_gpu((host[sl], rel[sl], od[sl], ids[sl], act[sl])))
                g = keep[-1]
                e.replay_device(g[0], g[1], g[2], g[3], g[4])
        res.append(_read(e))
        e.close()
    assert res[0][1] == [0]
    assert res[0][0][0][2] == c
    _close(res[0], res[1])


# ---- 7: the front-end in place ----

def _circle(T, phase=0.0):
    """Circle of radius 0.5 m about (0.1, 0) at 0.1 rad per message (tests/test_gpu_pipeline.py)."""
    a = phase + 0.1 * np.arange(T)
    return np.stack([a + math.pi / 2, 0.1 + 0.5 * np.cos(a), 0.5 * np.sin(a)], 1)


def _markers_to_messages(cnt, mk, T, F, M):
    c = np.clip(cnt, 0, M).astype(np.int32).reshape(T, F)
    rel = np.zeros((T, F, M, 2))
    rel[..., 0] = mk["x"].reshape(T, F, M)
    rel[..., 1] = mk["y"].reshape(T, F, M)
    return c, rel


def test_frontend_in_place_matches_host_hop_and_oracle(monkeypatch):
    """The 40-scan circle drive of tests/test_gpu_pipeline.py plus one scan with no cluster break
    and one with no detection (tests/golden/scans.npz): detect_device + replay_into against detect
    → host → replay(assoc=True); filter 0's pose within 1e-8 of the oracle pipeline. A second
    detect_device issued right behind replay_into must not disturb the replay."""
    from pyekf.landmarks import Detector, LM_NO_BREAK
    _env(monkeypatch)
    pyekf.poison_lds()
    g = np.load(GOLD)
    no_break, nothing = 25, 4
    assert g["counts"][no_break] == LM_NO_BREAK and g["counts"][nothing] == 0
    inc = float(np.float32(2 * math.pi / 360))
    p40 = _circle(40)
    s40 = synth.lidar_scans(p40, BASIC, sigma=0.001, seed=11)
    order = list(range(11)) + [-1] + list(range(11, 26)) + [-2] + list(range(26, 40))
    scans = np.stack([s40[k] if k >= 0 else g["ranges"][no_break if k == -1 else nothing, :360]
                      for k in order]).astype(np.float32)
    poses = np.stack([p40[k] if k >= 0 else p40[order[i - 1]] for i, k in enumerate(order)])
    amin = np.array([0.0 if k >= 0 else g["angle_min"][no_break if k == -1 else nothing]
                     for k in order])
    ainc = np.array([inc if k >= 0 else g["angle_inc"][no_break if k == -1 else nothing]
                     for k in order])
    T, M = len(order), 8
    # the oracle pipeline, margins asserted
    ref = orc.OracleEKF(n_landmarks=N)
    seen = 0
    for t in range(T):
        ref.set_odom(poses[t])
        want = L.laser_callback(scans[t], float(amin[t]), float(ainc[t]))
        if not want:
            continue  # no break / nothing detected: landmarks.cpp:153 publishes nothing
        seen += len(want)
        _oracle_message(ref, np.array([[w[1], w[2]] for w in want]))
    assert seen >= 20
    # in place
    det = Detector(max_scans=T, max_beams=360)
    ekf = pyekf.EKF(n_landmarks=N)
    assert det.detect_device(scans, amin, ainc, max_markers=M) == T
    assert det.replay_into(ekf, T, poses[:, None, :]) == pyekf.EKF_OK
    det.detect_device(scans[::-1], amin[::-1], ainc[::-1], max_markers=M)  # right behind it
    got = _read(ekf)
    ekf.close()
    # the host hop
    cnt, mk = det.detect(scans, amin, ainc, max_markers=M)
    assert cnt[order.index(-1)] == LM_NO_BREAK and cnt[order.index(-2)] == 0
    c, rel = _markers_to_messages(cnt, mk, T, 1, M)
    ekf = pyekf.EKF(n_landmarks=N)
    ekf.replay(c, rel, poses[:, None, :], assoc=True)
    want = _read(ekf)
    ekf.close()
    det.close()
    assert got[1] == [0]
    _close(got, want)
    xr, _, _, cr = ref.get(sigma=False)
    assert got[0][0][2] == cr >= 3
    assert np.abs(got[2][0] - xr[:3]).max() < 1e-8


def test_frontend_in_place_from_simulated_scans_two_robots(monkeypatch):
    """The same from lm_simulate's resident scans (ranges=None), F = 2 robots × 20 scans (scan
    t·F + f is message t of robot f), lm_marker rows read in place; lm_fetch_markers returns what
    lm_detect_resident does."""
    from pyekf.landmarks import Detector
    _env(monkeypatch)
    pyekf.poison_lds()
    T, F, M = 20, 2, 8
    poses = np.stack([_circle(T), _circle(T, 2.0)], 1)  # [T, F, 3]
    det = Detector(max_scans=T * F, max_beams=360)
    scans = det.simulate(poses.reshape(T * F, 3), BASIC, sigma=0.001, seed=11)
    inc = float(np.float32(2 * math.pi / 360))
    for f in range(F):  # the oracle pipeline of each robot, margins asserted
        ref = orc.OracleEKF(n_landmarks=N)
        for t in range(T):
            ref.set_odom(poses[t, f])
            want = L.laser_callback(scans[t * F + f], 0.0, inc)
            if want:
                _oracle_message(ref, np.array([[w[1], w[2]] for w in want]))
        if f == 0:
            ref0 = ref
    ekf = pyekf.EKF(n_landmarks=N, n_filters=F)
    assert det.detect_device(max_markers=M) == T * F
    cf, mf = det.fetch_markers()
    assert det.replay_into(ekf, T, poses) == pyekf.EKF_OK
    got = _read(ekf)
    ekf.close()
    cnt, mk = det.detect_resident(max_markers=M)
    np.testing.assert_array_equal(cf, cnt)
    assert mf.tobytes() == mk.tobytes()
    assert (cnt > 0).sum() >= 20
    c, rel = _markers_to_messages(cnt, mk, T, F, M)
    ekf = pyekf.EKF(n_landmarks=N, n_filters=F)
    ekf.replay(c, rel, poses, assoc=True)
    want = _read(ekf)
    ekf.close()
    det.close()
    assert got[1] == [0] * F
    _close(got, want)
    xr, _, _, cr = ref0.get(sigma=False)
    assert got[0][0][2] == cr >= 3
    assert np.abs(got[2][0] - xr[:3]).max() < 1e-8


# ---- 8: rejections ----

def _same(a, b):
    (sa, fa, pa), (sb, fb, pb) = a, b
    assert fa == fb
    for (xa, Sa, ca), (xb, Sb, cb) in zip(sa, sb):
        assert ca == cb
        np.testing.assert_array_equal(xa, xb)
        np.testing.assert_array_equal(Sa, Sb)


def test_rejections_change_nothing(monkeypatch):
    """EKF_E_ARG, and the state as it was: T < 1, m_max outside [1, 64], stride < 2, a NULL counts
    / xy / odom, a resident handle (N = 50), the one-marker route (EKF_ASSOC_MSG=0), nothing
    detected yet, a front-end / filter scan-count mismatch."""
    from pyekf.landmarks import Detector
    _env(monkeypatch)
    pyekf.poison_lds()
    dev, host, rel, od, _, _ = _case(1, 30, 16, 7, True)
    T, M = 4, 16
    g = _gpu((dev[:T], rel[:T], od[:T]))
    cp, xp, op = (t.data_ptr() for t in g)
    e = pyekf.EKF(n_landmarks=N)
    e.replay(host[:T], rel[:T], od[:T], assoc=True)
    before = _read(e)
    bad = [(0, M, cp, xp, 2, op), (-1, M, cp, xp, 2, op), (T, 0, cp, xp, 2, op),
           (T, 65, cp, xp, 2, op), (T, M, cp, xp, 1, op), (T, M, 0, xp, 2, op),
           (T, M, cp, 0, 2, op), (T, M, cp, xp, 2, 0)]
    for a in bad:
        assert e.replay_device_assoc_raw(*a) == pyekf.EKF_E_ARG, a
    import torch
    with pytest.raises(ValueError):  # neither packed pairs nor lm_marker rows
        e.replay_device_assoc(g[0], torch.zeros((T, 1, M, 3), dtype=torch.float64, device="cuda"),
                              g[2])
    det = Detector(max_scans=4, max_beams=360)
    assert det.replay_into(e, 4, np.zeros((4, 1, 3))) == pyekf.EKF_E_ARG  # nothing detected yet
    scans = synth.lidar_scans(_circle(3), BASIC, sigma=0.001, seed=11)
    inc = float(np.float32(2 * math.pi / 360))
    assert det.detect_device(scans, 0.0, inc, max_markers=8) == 3
    assert det.replay_into(e, 2, np.zeros((2, 1, 3))) == pyekf.EKF_E_ARG    # 3 scans ≠ T·F = 2
    _same(_read(e), before)
    assert e.replay_device_assoc_raw(T, M, cp, xp, 2, op) == pyekf.EKF_OK  # (the handle still runs)
    e.sync()
    assert e.status() == 0
    e.close()
    # a resident handle
    r = pyekf.EKF(n_landmarks=50)
    assert r.path == pyekf.EKF_PATH_RESIDENT
    r.set_odom(od[0, 0])
    r.sensor(rel[0, 0, :4], decisions=False)
    before = _read(r)
    assert r.replay_device_assoc_raw(T, M, cp, xp, 2, op) == pyekf.EKF_E_ARG
    assert det.replay_into(r, 3, np.zeros((3, 1, 3))) == pyekf.EKF_E_ARG
    _same(_read(r), before)
    r.close()
    # the one-marker route
    _env(monkeypatch, EKF_ASSOC_MSG="0")
    m = pyekf.EKF(n_landmarks=N)
    assert m.assoc_route == pyekf.EKF_ASSOC_MARKER
    m.replay(host[:T], rel[:T], od[:T], assoc=True)
    before = _read(m)
    assert m.replay_device_assoc_raw(T, M, cp, xp, 2, op) == pyekf.EKF_E_ARG
    assert det.replay_into(m, 3, np.zeros((3, 1, 3))) == pyekf.EKF_E_ARG
    _same(_read(m), before)
    m.close()
    det.close()
