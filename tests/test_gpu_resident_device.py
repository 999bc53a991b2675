"""ekf_replay_resident / lm_replay_resident (include/ekf.h, include/landmarks.h): replays on the
resident path (n <= 128, fp64) whose inputs already live on the GPU, walked by one launch of
k_resident_replay (ekf_resident.hip) with no descriptors.

Parity: the same messages through the host planner on a second resident handle (ekf_replay: the same
kernel phases in the same order), at the project's bounds for device- against host-planned replays
(tests/test_gpu_assoc_device.py): state and poses 1e-9, Σ 1e-8, counters, status words and
decisions exact. The two differ only in the last bit of a bearing, where glibc's atan2 on the host
is not the correctly rounded value the device computes (atan2_dd.hpp).

Against the CPU oracle no number is fixed: the device run may be as far from the oracle as the
host-planned resident run on the same drive is, plus 1e-9, on the state and on Σ alike.

Unknown-association drives are chosen by the margin method of tests/test_gpu_assoc_device.py: the
oracle alone runs first, marker by marker, and every decision must clear the gate and the runner-up
by 1e-6 relative (its _oracle_message asserts it), so a last-bit change of a bearing cannot flip
one."""
import functools
import math

import numpy as np
import pytest

import landmarks_numpy as L
import orc
import pyekf
from pyekf import synth

import test_gpu_assoc_device as tad  # _oracle_message: the margins of every decision

pytestmark = pytest.mark.gpu

STATE_TOL, SIGMA_TOL = 1e-9, 1e-8  # tests/test_gpu_assoc_device.py:41
ORACLE_SLACK = 1e-9  # over the host-planned run's own distance from the oracle
ENV = tad.ENV
BASIC = tad.BASIC


def _env(monkeypatch):
    for k in ENV:
        monkeypatch.delenv(k, raising=False)


def _gpu(arrs):
    import torch
    return tuple(None if a is None else torch.from_numpy(np.array(a, order="C")).cuda()
                 for a in arrs)


def _read(e):
    return ([e.state(f) for f in range(e.F)], [e.status(f) for f in range(e.F)],
            np.stack([e.pose(f) for f in range(e.F)]))


def _close(a, b, what="device- against host-planned"):
    (sa, fa, pa), (sb, fb, pb) = a, b
    print(what + ", per filter (state, sigma):",
          [(float(np.abs(xa - xb).max()), float(np.abs(Sa - Sb).max()))
           for (xa, Sa, _), (xb, Sb, _) in zip(sa, sb)])
    assert fa == fb
    for (xa, Sa, ca), (xb, Sb, cb) in zip(sa, sb):
        assert ca == cb
        assert np.all(np.isfinite(Sa))
        assert np.abs(xa - xb).max() <= STATE_TOL
        assert np.abs(Sa - Sb).max() <= SIGMA_TOL
    assert np.abs(pa - pb).max() <= STATE_TOL


def _same(a, b):
    (sa, fa, pa), (sb, fb, pb) = a, b
    assert fa == fb
    for (xa, Sa, ca), (xb, Sb, cb) in zip(sa, sb):
        assert ca == cb
        np.testing.assert_array_equal(xa, xb)
        np.testing.assert_array_equal(Sa, Sb)


def _within_oracle(dev, host, oracle):
    """dev, host: _read() results; oracle: per filter (x, S, counter). The device run is no
    farther from the oracle than the host-planned run, plus 1e-9."""
    for f, (xo, So, co) in enumerate(oracle):
        (xd, Sd, cd), (xh, Sh, ch) = dev[0][f], host[0][f]
        dx, hx = float(np.abs(xd - xo).max()), float(np.abs(xh - xo).max())
        dS, hS = float(np.abs(Sd - So).max()), float(np.abs(Sh - So).max())
        print(f"filter {f} against the oracle: state device {dx:.3e} host {hx:.3e}, "
              f"sigma device {dS:.3e} host {hS:.3e}")
        assert cd == ch == co
        assert dx <= hx + ORACLE_SLACK
        assert dS <= hS + ORACLE_SLACK


def _resident(N, F, joseph=False):
    e = pyekf.EKF(n_landmarks=N, n_filters=F)
    assert e.path == pyekf.EKF_PATH_RESIDENT
    if joseph:
        assert e.set_joseph(True) == pyekf.EKF_OK
    return e


# ---- 1: known ids ----

@functools.lru_cache(maxsize=None)
def _known_case(N, T, joseph=False, F=3, M=6, seed=5):
    """F robots × T messages of at most M markers with known ids (robot f: synth.synthetic seed +
    f, the 5 nearest landmarks plus one DELETE marker). Filter 1 sits steps out (count 0 and −1),
    one message of filter 2 is all DELETE (predict + posterior), one full message of filter 0
    reports more markers than M. Returns the device counts, the host's (clamped to [0, M]), ids,
    actions, rel, odom and the oracle's end (x, Σ, counter) per filter."""
    cnt = np.zeros((T, F), np.int32)
    ids = np.zeros((T, F, M), np.int32)
    act = np.zeros((T, F, M), np.int32)
    rel = np.zeros((T, F, M, 2))
    od = np.zeros((T, F, 3))
    for f in range(F):
        sc = synth.synthetic(N, T, seed=seed + f, max_markers=M - 1, n_delete=1)
        assert sc.ids.shape[1] == M
        cnt[:, f], ids[:, f], act[:, f], rel[:, f] = sc.count, sc.ids, sc.actions, sc.rel
        od[:, f] = pyekf.odometry(sc)
    assert (act == pyekf.DELETE).any()
    ids = np.maximum(ids, 0)  # (slots beyond a message's count: never read)
    act[1::4, 0, 1] = pyekf.DELETE  # (in mid-list too: the markers behind it move up)
    if T > 2:
        act[T // 2, F - 1, :] = pyekf.DELETE
    dev = cnt.copy()
    dev[1::3, 1] = 0
    dev[2::6, 1] = -1
    full = np.flatnonzero(cnt[:, 0] == M)
    assert full.size
    dev[full[full.size // 2], 0] = M + 3
    host = np.clip(dev, 0, M).astype(np.int32)
    oracle = []
    for f in range(F):
        ref = orc.OracleEKF(n_landmarks=N, joseph=joseph)
        for t in range(T):
            c = int(host[t, f])
            if c:
                ref.set_odom(od[t, f])
                assert ref.fake_sensor_cb(ids[t, f, :c], act[t, f, :c], rel[t, f, :c]) == 0
        x, S, _, k = ref.get()
        oracle.append((x, S, k))
    for a in (dev, host, ids, act, rel, od):
        a.setflags(write=False)
    return dev, host, ids, act, rel, od, oracle


def _run_known(kind, N, case, joseph, sl=slice(None)):
    dev, host, ids, act, rel, od, _ = case
    e = _resident(N, dev.shape[1], joseph)
    if kind == "device":
        g = _gpu((dev[sl], rel[sl], od[sl], ids[sl], act[sl]))
        e.replay_resident(g[0], g[1], g[2], ids=g[3], actions=g[4])
    else:
        e.replay(host[sl], rel[sl], od[sl], ids=ids[sl], actions=act[sl])
    out = _read(e)
    e.close()
    return out


@pytest.mark.parametrize("joseph", [False, True], ids=["simple", "joseph"])
@pytest.mark.parametrize("N,T", [(20, 17), (62, 17), (50, 1), (50, 7), (50, 8), (50, 9), (50, 17),
                                 (50, 33)])
def test_known_ids_equal_host_replay(monkeypatch, N, T, joseph):
    """N = 20, 50, 62 (n = 43, 103, 127: one per kernel shape), F = 3, m_max = 6, both forms; T
    on either side of every staging-block boundary. Filter 1 sits steps out, DELETE markers are
    compacted away, one message is all DELETE, one count is above m_max."""
    _env(monkeypatch)
    pyekf.poison_lds()
    case = _known_case(N, T, joseph)
    d = _run_known("device", N, case, joseph)
    h = _run_known("host", N, case, joseph)
    assert d[1] == [0, 0, 0]
    _close(d, h)
    _within_oracle(d, h, case[6])
    assert all(np.abs(s[0][3:]).max() > 0 for s in d[0])  # landmarks were initialised


def test_known_id_out_of_range_is_skipped_and_flagged(monkeypatch):
    """The inputs are not validated on the host: an id outside [0, N) is skipped and sets
    EKF_FLAG_RANGE. The rest equals the host-planned run with those markers marked DELETE."""
    _env(monkeypatch)
    pyekf.poison_lds()
    dev, host, ids, act, rel, od, _ = _known_case(50, 9)
    bad_ids, del_act = ids.copy(), act.copy()
    for t, f, i, v in ((2, 0, 0, 50), (6, 2, 3, -1), (6, 2, 0, 1 << 30)):
        assert act[t, f, i] != pyekf.DELETE and i < host[t, f]
        bad_ids[t, f, i] = v
        del_act[t, f, i] = pyekf.DELETE
    e = _resident(50, 3)
    g = _gpu((dev, rel, od, bad_ids, act))
    e.replay_resident(g[0], g[1], g[2], ids=g[3], actions=g[4])
    d = _read(e)
    e.close()
    e = _resident(50, 3)
    e.replay(host, rel, od, ids=ids, actions=del_act)
    h = _read(e)
    e.close()
    assert d[1] == [pyekf.EKF_FLAG_RANGE, 0, pyekf.EKF_FLAG_RANGE]
    _close((d[0], [0, 0, 0], d[2]), h)


# ---- 2: unknown association ----

def _oracle_assoc_drive(N, cnt, rel, od, joseph):
    ref = orc.OracleEKF(n_landmarks=N, joseph=joseph)
    dec = []
    for t in range(len(cnt)):
        c = max(int(cnt[t]), 0)
        if c:
            ref.set_odom(od[t])
        dec.append(tad._oracle_message(ref, rel[t, :c]))
    x, S, _, k = ref.get()
    return (x, S, k), dec


ASSOC_SEED = {16: 1, 33: 1}  # drives whose every decision clears the margins (found on the CPU)


@functools.lru_cache(maxsize=None)
def _assoc_case(M, joseph=False, N=50, F=2, T=12, n_map=40):
    """F robots × T messages of at most M shuffled markers without ids, over maps of n_map
    landmarks in N slots. M > 17: messages of 17 to M markers in turn. Filter 1 sits steps out,
    one full message of filter 0 reports more markers than M."""
    seed = ASSOC_SEED[M]
    cnt = np.zeros((T, F), np.int32)
    rel = np.zeros((T, F, M, 2))
    od = np.zeros((T, F, 3))
    for f in range(F):
        sc = synth.make_scenario(N, synth.random_landmarks(n_map, seed + f), T, seed=seed + f,
                                 max_markers=M, shuffle=True)
        cnt[:, f] = sc.count
        if M > 17:
            cnt[:, f] = np.minimum(sc.count, np.roll([M, 17, 25], f)[np.arange(T) % 3])
        rel[:, f] = sc.rel
        od[:, f] = pyekf.odometry(sc)
    dev = cnt.copy()
    dev[1::3, 1] = 0
    dev[2::6, 1] = -1
    full = np.flatnonzero(cnt[:, 0] == M)
    assert full.size
    dev[full[full.size // 2], 0] = M + 5
    host = np.clip(dev, 0, M).astype(np.int32)
    runs = [_oracle_assoc_drive(N, host[:, f], rel[:, f], od[:, f], joseph) for f in range(F)]
    for a in (dev, host, rel, od):
        a.setflags(write=False)
    return dev, host, rel, od, [r[0] for r in runs], [r[1] for r in runs]


def _xy4(rel):
    """lm_marker rows (x, y, r, id/pad): what the kernel must not read is NaN."""
    xy = np.full(rel.shape[:-1] + (4,), np.nan)
    xy[..., :2] = rel
    return xy


@pytest.mark.parametrize("stride", [2, 4])
@pytest.mark.parametrize("joseph", [False, True], ids=["simple", "joseph"])
@pytest.mark.parametrize("M", [16, 33])
def test_unknown_association_equals_host_replay(monkeypatch, M, joseph, stride):
    """N = 50, F = 2, m_max = 16 and 33 (decision slots beyond 16), packed pairs and lm_marker
    rows, both forms: state, Σ, counters and status against the host-planned replay, the last
    message's decisions against it and the oracle."""
    _env(monkeypatch)
    pyekf.poison_lds()
    dev, host, rel, od, oracle, dec = _assoc_case(M, joseph)
    if M > 17:
        assert host.max() == M and (host[host > 0] >= 17).all()
    res, decs = [], []
    keep = None
    for kind in ("device", "host"):
        e = _resident(50, 2, joseph)
        if kind == "device":
            keep = _gpu((dev, rel if stride == 2 else _xy4(rel), od))
            e.replay_resident(*keep)
        else:
            e.replay(host, rel, od, assoc=True)
        res.append(_read(e))
        decs.append([e.decisions(M, f) for f in range(2)])
        e.close()
    d, h = res
    assert d[1] == [0, 0]
    _close(d, h)
    _within_oracle(d, h, oracle)
    for f in range(2):
        np.testing.assert_array_equal(decs[0][f][0], decs[1][f][0])
        np.testing.assert_array_equal(decs[0][f][1], decs[1][f][1])
        last = max(t for t in range(host.shape[0]) if host[t, f] > 0)
        c = int(host[last, f])
        np.testing.assert_array_equal(decs[0][f][0][:c], dec[f][last][0])
        np.testing.assert_array_equal(decs[0][f][1][:c], dec[f][last][1])
    assert any(dd[1].any() for dd in dec[0]) and not all(dd[1].all() for dd in dec[0] if len(dd[1]))


# ---- 3: one launch ----

def test_one_launch_per_replay(monkeypatch):
    """A 33-message replay is one launch of the resident kernel slot and none of the pipeline's."""
    _env(monkeypatch)
    dev, host, ids, act, rel, od, _ = _known_case(50, 33)
    e = _resident(50, 3)
    e.profile(True)
    g = _gpu((dev, rel, od, ids, act))
    e.replay_resident(g[0], g[1], g[2], ids=g[3], actions=g[4])
    e.sync()
    n, ms = e.profile_read(4)
    print(f"k_resident_replay, 33 messages x 3 filters: {1e3 * ms:.1f} us")
    assert n == 1 and ms > 0.0
    for k in range(4):
        assert e.profile_read(k)[0] == 0
    e.close()


# ---- 4: the pose trace ----

def test_trace_records_every_active_message(monkeypatch):
    """trace_enable(40), T = 33: a filter's records are its messages with count > 0 (the all-DELETE
    one included), seq 0, 1, …, poses and t_map_odom as the host-planned traced run's."""
    _env(monkeypatch)
    pyekf.poison_lds()
    case = _known_case(50, 33)
    dev, host, ids, act, rel, od, _ = case
    tr = []
    for kind in ("device", "host"):
        e = _resident(50, 3)
        e.trace_enable(40)
        if kind == "device":
            g = _gpu((dev, rel, od, ids, act))
            e.replay_resident(g[0], g[1], g[2], ids=g[3], actions=g[4])
        else:
            e.replay(host, rel, od, ids=ids, actions=act)
        tr.append([(e.trace_count(f),) + e.trace(f) for f in range(3)])
        e.close()
    for f in range(3):
        (nd, pd, md, sd), (nh, ph, mh, sh) = tr[0][f], tr[1][f]
        active = int((host[:, f] > 0).sum())
        assert nd == nh == active == len(sd)
        np.testing.assert_array_equal(sd, np.arange(active))
        print(f"filter {f} trace, device- against host-planned: pose "
              f"{float(np.abs(pd - ph).max()):.3e} map_odom {float(np.abs(md - mh).max()):.3e}")
        assert np.abs(pd - ph).max() <= STATE_TOL
        assert np.abs(md - mh).max() <= STATE_TOL
    assert (host[:, 1] > 0).sum() < 33


# ---- 5: chaining with host-planned calls ----

def test_chaining_with_host_planned_calls(monkeypatch):
    """device replay → ekf_sensor (host-planned) → device replay → state read equals the all-host
    run. In the second replay filter 1 gets no message: bit-identical to before, Σ included. A
    pending ekf_predict survives a replay that holds no message for its filter."""
    _env(monkeypatch)
    pyekf.poison_lds()
    dev, host, rel, od, _, _ = _assoc_case(16)
    a, b = slice(0, 5), slice(6, 12)
    dev2, host2 = dev[b].copy(), host[b].copy()
    dev2[:, 1] = [0, -1, 0, 0, -1, 0]
    host2[:, 1] = 0
    res, mid = [], []
    keep = []
    for kind in ("device", "host"):
        e = _resident(50, 2)
        if kind == "device":
            keep.append(_gpu((dev[a], rel[a], od[a])))
            e.replay_resident(*keep[-1])
        else:
            e.replay(host[a], rel[a], od[a], assoc=True)
        for f in range(2):  # message 5 through ekf_sensor, no decisions asked for
            e.set_odom(od[5, f], f)
            assert e.sensor(rel[5, f, :int(host[5, f])], f=f, decisions=False)[0] == pyekf.EKF_OK
        mid.append(_read(e))
        if kind == "device":
            keep.append(_gpu((dev2, rel[b], od[b])))
            e.replay_resident(*keep[-1])
        else:
            e.replay(host2, rel[b], od[b], assoc=True)
        res.append(_read(e))
        e.close()
    assert host[5].min() > 0
    assert res[0][1] == [0, 0]
    _close(mid[0], mid[1], "after the replay and ekf_sensor")
    _close(res[0], res[1], "after the second replay")
    np.testing.assert_array_equal(res[0][0][1][0], mid[0][0][1][0])  # filter 1: nothing changed
    np.testing.assert_array_equal(res[0][0][1][1], mid[0][0][1][1])
    assert np.abs(res[0][0][0][0] - mid[0][0][0][0]).max() > 0      # filter 0 moved on
    # a pending predict: device replay with no message for filter 1, then a correction
    kdev, khost, ids, act, krel, kod, _ = _known_case(50, 7)
    cd, ch = kdev.copy(), khost.copy()
    cd[:, 1] = -1
    ch[:, 1] = 0
    out = []
    for kind in ("device", "host", "not_pending"):
        e = _resident(50, 3)
        e.replay(khost[:3], krel[:3], kod[:3], ids=ids[:3], actions=act[:3])
        if kind != "not_pending":
            assert e.predict(1) == pyekf.EKF_OK
        if kind == "device":
            g = _gpu((cd[3:], krel[3:], kod[3:], ids[3:], act[3:]))
            e.replay_resident(g[0], g[1], g[2], ids=g[3], actions=g[4])
        else:
            e.replay(ch[3:], krel[3:], kod[3:], ids=ids[3:], actions=act[3:])
        assert e.correct(int(ids[0, 1, 0]), 0.7, -0.4, f=1) == pyekf.EKF_OK
        out.append(_read(e))
        e.close()
    _close(out[0], out[1], "pending predict kept")
    np.testing.assert_array_equal(out[0][0][1][0], out[1][0][1][0])
    np.testing.assert_array_equal(out[0][0][1][1], out[1][0][1][1])
    assert np.abs(out[0][0][1][1] - out[2][0][1][1]).max() > 0  # (the predict does show)


# ---- 6: a full map ----

@pytest.mark.parametrize("T", [1, 6])
def test_full_map_flags_and_decisions(monkeypatch, T):
    """N = 4 slots (n = 11), six distinct landmarks: a marker that meets the full map is skipped
    with decision −1 and EKF_FLAG_RANGE, as in the host-planned run. T = 1: four markers open the
    four slots, the two behind them are refused. T = 6: the last message meets a map that is full
    already, where associate_correct refuses every marker before scoring it (the reference indexes
    out of range there, slam.cpp:351)."""
    _env(monkeypatch)
    pyekf.poison_lds()
    lm = np.array([(1.5, 0.2), (-1.4, 0.9), (0.3, 1.8), (0.2, -1.7), (2.0, -1.5), (-1.9, -1.2)])
    M = 6
    sc = synth.make_scenario(6, lm, T, max_markers=M, shuffle=True, seed=9)
    assert (sc.count == M).all()
    cnt = sc.count[:, None].astype(np.int32)
    rel, od = sc.rel[:, None], pyekf.odometry(sc)[:, None]
    res = []
    for kind in ("device", "host"):
        e = _resident(4, 1)
        if kind == "device":
            g = _gpu((cnt, rel, od))
            e.replay_resident(*g)
        else:
            e.replay(cnt, rel, od, assoc=True)
        dec = e.decisions(M)
        res.append((_read(e), dec))
        e.close()
    (d, dd), (h, hd) = res
    assert d[1] == h[1] == [pyekf.EKF_FLAG_RANGE]
    assert d[0][0][2] == h[0][0][2] == 4
    np.testing.assert_array_equal(dd[0], hd[0])
    np.testing.assert_array_equal(dd[1], hd[1])
    if T == 1:
        np.testing.assert_array_equal(dd[0], [0, 1, 2, 3, -1, -1])
        np.testing.assert_array_equal(dd[1], [1, 1, 1, 1, 0, 0])
    else:
        assert (dd[0] == -1).all() and not dd[1].any()
    _close(d, h)


# ---- 7: the front-end in place ----

def test_frontend_simulated_scans_into_resident_filter(monkeypatch):
    """lm_simulate (2 robots × 10 scans, 360 beams, the BASIC scene) → detect_device(8) →
    replay_resident at N = 50, against fetch_markers + the host replay on a second resident handle
    and the oracle pipeline; a second detect_device right behind it must not disturb the replay."""
    from pyekf.landmarks import Detector
    _env(monkeypatch)
    pyekf.poison_lds()
    T, F, M, N = 10, 2, 8, 50
    poses = np.stack([tad._circle(T), tad._circle(T, 2.0)], 1)  # [T, F, 3]
    det = Detector(max_scans=T * F, max_beams=360)
    scans = det.simulate(poses.reshape(T * F, 3), BASIC, sigma=0.001, seed=11)
    inc = float(np.float32(2 * math.pi / 360))
    oracle = []
    for f in range(F):  # the oracle pipeline of each robot, margins asserted
        ref = orc.OracleEKF(n_landmarks=N)
        for t in range(T):
            ref.set_odom(poses[t, f])
            want = L.laser_callback(scans[t * F + f], 0.0, inc)
            if want:
                tad._oracle_message(ref, np.array([[w[1], w[2]] for w in want]))
        x, S, _, k = ref.get()
        oracle.append((x, S, k))
    ekf = _resident(N, F)
    assert det.detect_device(max_markers=M) == T * F
    cf, mf = det.fetch_markers()
    assert det.replay_resident(ekf, T, poses) == pyekf.EKF_OK
    det.detect_device(scans[::-1], 0.0, inc, max_markers=M)  # right behind it
    got = _read(ekf)
    ekf.close()
    assert (cf > 0).sum() >= 10
    c, rel = tad._markers_to_messages(cf, mf, T, F, M)
    ekf = _resident(N, F)
    ekf.replay(c, rel, poses, assoc=True)
    want = _read(ekf)
    ekf.close()
    det.close()
    assert got[1] == [0] * F
    _close(got, want)
    _within_oracle(got, want, oracle)
    assert min(s[2] for s in got[0]) >= 2  # (ten scans of this circle show two or three cylinders)


def test_replay_on_device_picks_the_pipeline_entry_points(monkeypatch):
    """EKF.replay_on_device on a pipeline handle (N = 96): known ids go through
    ekf_replay_device, no ids through ekf_replay_device_assoc, each bit-identical to the direct
    call; lm_marker rows with known ids are refused (that entry point takes packed pairs)."""
    import torch
    _env(monkeypatch)
    pyekf.poison_lds()
    _, host, ids, act, rel, od, _ = _known_case(50, 7)
    g = _gpu((host, rel, od, ids, act))
    res = []
    for via in (True, False):
        e = pyekf.EKF(n_landmarks=96, n_filters=3)
        assert e.path == pyekf.EKF_PATH_PIPELINE
        if via:
            with pytest.raises(ValueError):
                e.replay_on_device(g[0], torch.zeros((7, 3, 6, 4), dtype=torch.float64,
                                                     device="cuda"), g[2], ids=g[3])
            e.replay_on_device(g[0], g[1], g[2], ids=g[3], actions=g[4])
        else:
            e.replay_device(g[0], g[1], g[2], g[3], g[4])
        res.append(_read(e))
        e.close()
    assert res[0][1] == [0, 0, 0]
    _same(res[0], res[1])
    dev, _, arel, aod, _, _ = _assoc_case(16)
    ga = _gpu((dev, arel, aod))
    res = []
    for via in (True, False):
        e = pyekf.EKF(n_landmarks=96, n_filters=2)
        assert e.assoc_route != pyekf.EKF_ASSOC_MARKER
        (e.replay_on_device if via else e.replay_device_assoc)(*ga)
        res.append(_read(e))
        e.close()
    assert res[0][1] == [0, 0] and min(s[2] for s in res[0][0]) > 0
    _same(res[0], res[1])


# ---- 8: rejections ----

def test_rejections_change_nothing(monkeypatch):
    """EKF_E_ARG and the state as it was, bit for bit: a NULL counts / xy / odom, known ids
    without ids, T < 1, m_max outside [1, 64], xy_stride < 2, what lm_replay_into lists, a NULL
    handle; a pipeline handle (N = 96). The resident handle still runs afterwards."""
    from pyekf.landmarks import Detector
    _env(monkeypatch)
    dev, host, ids, act, rel, od, _ = _known_case(50, 7)
    T, M = 4, 6
    g = _gpu((dev[:T], rel[:T], od[:T], ids[:T], act[:T]))
    cp, xp, op, ip, ap = (t.data_ptr() for t in g)
    e = _resident(50, 3)
    e.replay(host[:T], rel[:T], od[:T], ids=ids[:T], actions=act[:T])
    before = _read(e)
    bad = [(0, T, M, 0, ip, ap, xp, 2, op), (0, T, M, cp, ip, ap, 0, 2, op),
           (0, T, M, cp, ip, ap, xp, 2, 0), (0, T, M, cp, 0, ap, xp, 2, op),
           (1, T, M, 0, 0, 0, xp, 2, op), (0, 0, M, cp, ip, ap, xp, 2, op),
           (1, -1, M, cp, 0, 0, xp, 2, op), (0, T, 0, cp, ip, ap, xp, 2, op),
           (1, T, 65, cp, 0, 0, xp, 2, op), (0, T, M, cp, ip, ap, xp, 1, op)]
    for a in bad:
        assert e.replay_resident_raw(*a) == pyekf.EKF_E_ARG, a
    L_ = pyekf.lib()
    assert L_.ekf_replay_resident(None, 0, T, M, cp, ip, ap, xp, 2, op) == pyekf.EKF_E_ARG
    det = Detector(max_scans=6, max_beams=360)
    assert det.replay_resident(e, 2, np.zeros((2, 3, 3))) == pyekf.EKF_E_ARG  # nothing detected yet
    scans = synth.lidar_scans(tad._circle(6), BASIC, sigma=0.001, seed=11)
    inc = float(np.float32(2 * math.pi / 360))
    assert det.detect_device(scans, 0.0, inc, max_markers=8) == 6
    assert det.replay_resident(e, 1, np.zeros((1, 3, 3))) == pyekf.EKF_E_ARG  # 6 scans ≠ T·F = 3
    assert L_.lm_replay_resident(det.h, None, 2, od.ctypes.data) == pyekf.EKF_E_ARG
    assert L_.lm_replay_resident(det.h, e.h, 0, od.ctypes.data) == pyekf.EKF_E_ARG
    assert L_.lm_replay_resident(det.h, e.h, 2, None) == pyekf.EKF_E_ARG
    _same(_read(e), before)
    # a pipeline handle
    p = pyekf.EKF(n_landmarks=96, n_filters=3)
    assert p.path == pyekf.EKF_PATH_PIPELINE
    p.replay(host[:T], rel[:T], od[:T], ids=ids[:T], actions=act[:T])
    pb = _read(p)
    assert p.replay_resident_raw(0, T, M, cp, ip, ap, xp, 2, op) == pyekf.EKF_E_ARG
    assert p.replay_resident_raw(1, T, M, cp, 0, 0, xp, 2, op) == pyekf.EKF_E_ARG
    assert det.replay_resident(p, 2, np.zeros((2, 3, 3))) == pyekf.EKF_E_ARG
    _same(_read(p), pb)
    p.close()
    # ... and the resident handle still runs: the rest of the drive on the device
    g2 = _gpu((dev[T:], rel[T:], od[T:], ids[T:], act[T:]))
    e.replay_on_device(g2[0], g2[1], g2[2], ids=g2[3], actions=g2[4])
    after = _read(e)
    e.close()
    det.close()
    assert after[1] == [0, 0, 0]
    _close(after, _run_known("host", 50, _known_case(50, 7), False), "the drive, host then device")
