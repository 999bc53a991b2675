"""The pose trace (include/ekf.h ekf_trace_*, include/slam_core.h slam_replay_trace): every kernel
that stores a filter's posterior t_map_odom (k_chain, k_assoc_msg, k_resident, k_posterior) appends
the posterior pose and t_map_odom to a per-filter buffer on the device — the per-message outputs of
the reference node (nuslam/src/slam.cpp:273-291) without a synchronisation per message.

Tolerances are the project's own: fp64 poses and t_map_odom within 1e-8 of the C
oracle; everything else (counts, sequence numbers, trace against trace, trace against the
handle's own pose) is exact. Every drive moves the robot between messages (synth circle drives),
so a record in the wrong slot misses by centimetres."""
import ctypes as C
import math

import numpy as np
import pytest

import orc
import pyekf
from pyekf import synth

pytestmark = pytest.mark.gpu

TOL = 1e-8
ENV = ("EKF_SERIAL", "EKF_CU_SPLIT", "EKF_DEVSYNC", "EKF_AM_XCD", "EKF_ASSOC_MSG", "EKF_STAGE",
       "EKF_RESIDENT", "EKF_SIM_PARALLEL")


def _env(monkeypatch, **kv):
    for k in ENV:
        monkeypatch.delenv(k, raising=False)
    for k, v in kv.items():
        monkeypatch.setenv(k, v)


def _gpu(arrs):
    import torch
    return tuple(torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in arrs)


def _oracle_trace(N, cnt, rel, od, ids=None, act=None, joseph=False):
    """One filter's messages (cnt[t] <= 0: none) through the C oracle: the posterior pose and
    t_map_odom after each message it takes, [k, 3] each. ids = None: sensor_cb."""
    ref = orc.OracleEKF(n_landmarks=N, joseph=joseph)
    poses, tmo = [], []
    for t in range(len(cnt)):
        c = int(cnt[t])
        if c <= 0:
            continue
        ref.set_odom(od[t])
        if ids is None:
            rc, _, _ = ref.sensor_cb(rel[t, :c])
        else:
            rc = ref.fake_sensor_cb(ids[t, :c], act[t, :c], rel[t, :c])
        assert rc == 0
        x, _, tm, _ = ref.get(sigma=False)
        poses.append(x[:3].copy())
        tmo.append(tm.copy())
    return np.array(poses), np.array(tmo)


def _moves(poses):
    """The drive moves between records: a record one slot off would miss by centimetres."""
    assert np.abs(np.diff(poses[:, 1:], axis=0)).max(axis=1).min() > 1e-3


def _same_trace(a, b):
    for x, y in zip(a, b):
        np.testing.assert_array_equal(x, y)


# ---- 1: resident, one launch, many messages ----

@pytest.mark.parametrize("kind", ["known", "assoc", "joseph"])
def test_resident_one_launch(monkeypatch, kind):
    """N = 50 (k_resident), basic_world(24) deferred into one launch, capacity 32: 24 records with
    seq 0..23, each within 1e-8 of the oracle's per-message pose and t_map_odom, the last one the
    handle's own pose and t_map_odom bit for bit; in two halves with a flush between them the
    sequence continues; with F = 3 a filter that sits four messages out has 20."""
    _env(monkeypatch)
    assoc, joseph = kind == "assoc", kind == "joseph"
    T = 24
    sc = synth.basic_world(T, shuffle=assoc)
    od = pyekf.odometry(sc)
    o = orc.run_scenario(sc, assoc, joseph=joseph)
    assert not o["rcs"].any()
    _moves(o["poses"])
    cnt, rel = sc.count[:, None], sc.rel[:, None]
    ids = None if assoc else sc.ids[:, None]
    act = None if assoc else sc.actions[:, None]

    def drive(e, a, b, c=None):
        sl = slice(a, b)
        F = e.F
        rep = lambda x: None if x is None else np.repeat(x[sl], F, axis=1)  # noqa: E731
        e.replay(rep(cnt) if c is None else c[sl], rep(rel), np.repeat(od[sl, None], F, axis=1),
                 ids=rep(ids), actions=rep(act), assoc=assoc)

    def handle(F=1):
        e = pyekf.EKF(n_landmarks=50, n_filters=F)
        assert e.path == pyekf.EKF_PATH_RESIDENT
        if joseph:
            assert e.set_joseph(True) == pyekf.EKF_OK
        e.trace_enable(32)
        e.profile(True)
        e.defer(True)
        return e

    e = handle()
    drive(e, 0, T)
    assert e.trace_count() == T
    assert e.profile_read(4)[0] == 1  # the whole drive was one k_resident launch
    pose, tmo, seq = e.trace()
    np.testing.assert_array_equal(seq, np.arange(T))
    print("resident", kind, "max |pose - oracle|", np.abs(pose - o["poses"]).max(),
          "max |tmo - oracle|", np.abs(tmo - o["tmo"]).max())
    assert np.abs(pose - o["poses"]).max() < TOL
    assert np.abs(tmo - o["tmo"]).max() < TOL
    np.testing.assert_array_equal(pose[-1], e.pose())
    np.testing.assert_array_equal(tmo[-1], e.map_odom())
    assert e.status() == 0
    e.close()
    # two uploads: the sequence continues
    e = handle()
    drive(e, 0, T // 2)
    e.flush()
    drive(e, T // 2, T)
    assert e.trace_count() == T
    assert e.profile_read(4)[0] == 2
    pose2, tmo2, seq2 = e.trace()
    np.testing.assert_array_equal(seq2, np.arange(T))
    assert np.abs(pose2 - o["poses"]).max() < TOL and np.abs(tmo2 - o["tmo"]).max() < TOL
    e.close()
    # three filters, filter 1 sits four messages out
    c3 = np.repeat(cnt, 3, axis=1).astype(np.int32)
    out = [3, 4, 11, 20]
    c3[out, 1] = 0
    e = handle(3)
    drive(e, 0, T, c3)
    assert [e.trace_count(f) for f in range(3)] == [T, T - 4, T]
    for f in (0, 2):
        _same_trace(e.trace(f), (pose, tmo, seq))
    p1, t1, s1 = e.trace(1)
    np.testing.assert_array_equal(s1, np.arange(T - 4))
    np.testing.assert_array_equal(p1[-1], e.pose(1))
    np.testing.assert_array_equal(t1[-1], e.map_odom(1))
    np.testing.assert_array_equal(p1[:3], pose[:3])  # (the same drive until its first hole)
    e.close()


# ---- 2, 3: the pipeline, device-planned ----

def _known_inputs(F, T, seed, holes=True, max_markers=12):
    """Filter f: synth.synthetic(96) seed + f % 3, messages of 12, 5, 8, 9 and 1 markers in turn;
    holes: filter 1 gets no message at t = 2 and 7, the last filter's message 5 is all DELETE."""
    scs = []
    for k in range(min(F, 3)):
        s0 = synth.synthetic(96, T, seed=seed + k, max_markers=max_markers)
        cnt = np.minimum(s0.count, np.roll([12, 5, 8, 9, 1], k)[np.arange(T) % 5])
        scs.append((s0, cnt.astype(np.int32)))
    M = max_markers
    cnt = np.zeros((T, F), np.int32)
    ids = np.zeros((T, F, M), np.int32)
    act = np.zeros((T, F, M), np.int32)
    rel = np.zeros((T, F, M, 2))
    od = np.zeros((T, F, 3))
    for f in range(F):
        s, c = scs[f % len(scs)]
        cnt[:, f], ids[:, f], act[:, f], rel[:, f] = c, s.ids, s.actions, s.rel
        od[:, f] = pyekf.odometry(s)
    if holes:
        cnt[[t for t in (2, 7) if t < T], 1] = 0
        act[5, F - 1] = synth.DELETE
    return cnt, ids, act, rel, od


def _device_replay(N, F, arrs, T=None, dtype=pyekf.EKF_F64, cap=32):
    """replay_device of the first T messages on a fresh tracing handle → (traces per filter, counts,
    poses, t_map_odom per filter, status)."""
    cnt, ids, act, rel, od = (a[:T] for a in arrs)
    e = pyekf.EKF(n_landmarks=N, n_filters=F, dtype=dtype)
    assert e.path == pyekf.EKF_PATH_PIPELINE
    e.trace_enable(cap)
    g = _gpu((cnt, ids, act, rel, od))
    e.replay_device(g[0], g[3], g[4], g[1], g[2])
    counts = [e.trace_count(f) for f in range(F)]
    tr = [e.trace(f) for f in range(F)]
    end = [(e.pose(f), e.map_odom(f)) for f in range(F)]
    st = [e.status(f) for f in range(F)]
    e.close()
    return tr, counts, end, st


def test_pipeline_device_planned_schedules(monkeypatch):
    """N = 96 fp64, F = 4, T = 16 through ekf_replay_device (one persistent chain launch): each
    filter's count is its active messages, filter 0 and the filter with holes are within 1e-8 of
    the oracle, and the device-epoch, event and single-stream schedules give the same bits."""
    F, T = 4, 16
    arrs = _known_inputs(F, T, 7)
    cnt, ids, act, rel, od = arrs
    assert cnt.max() == 12 and cnt[cnt > 0].min() == 1
    assert (act[5, F - 1, :cnt[5, F - 1]] == synth.DELETE).all()
    runs = {}
    for name, env in (("default", {}), ("events", {"EKF_DEVSYNC": "0"}),
                      ("serial", {"EKF_SERIAL": "1"})):
        _env(monkeypatch, **env)
        pyekf.poison_lds()
        runs[name] = _device_replay(96, F, arrs)
    tr, counts, end, st = runs["default"]
    assert st == [0] * F
    assert counts == [int((cnt[:, f] > 0).sum()) for f in range(F)] == [16, 14, 16, 16]
    for f in range(F):
        np.testing.assert_array_equal(tr[f][2], np.arange(counts[f]))
        np.testing.assert_array_equal(tr[f][0][-1], end[f][0])
        np.testing.assert_array_equal(tr[f][1][-1], end[f][1])
    for f in (0, 1):
        po, to = _oracle_trace(96, cnt[:, f], rel[:, f], od[:, f], ids[:, f], act[:, f])
        _moves(po)
        print("filter", f, "max |pose - oracle|", np.abs(tr[f][0] - po).max(),
              "max |tmo - oracle|", np.abs(tr[f][1] - to).max())
        assert np.abs(tr[f][0] - po).max() < TOL
        assert np.abs(tr[f][1] - to).max() < TOL
    for name in ("events", "serial"):
        assert runs[name][1] == counts and runs[name][3] == st
        for f in range(F):
            _same_trace(runs[name][0][f], tr[f])


def test_pipeline_device_planned_36_filters(monkeypatch):
    """F = 36, T = 6: above 32 filters one stream is the default; its traces equal the two-stream
    (EKF_SERIAL=0, HIP events) run's bit for bit."""
    F, T = 36, 6
    arrs = _known_inputs(F, T, 51)
    cnt = arrs[0]
    runs = []
    for env in ({}, {"EKF_SERIAL": "0"}):
        _env(monkeypatch, **env)
        pyekf.poison_lds()
        runs.append(_device_replay(96, F, arrs, cap=8))
    (tr, counts, end, st), (tr2, counts2, _, st2) = runs
    assert st == st2 == [0] * F
    assert counts == counts2 == [int((cnt[:, f] > 0).sum()) for f in range(F)]
    assert counts[1] == T - 1 and counts[0] == T
    for f in range(F):
        np.testing.assert_array_equal(tr[f][2], np.arange(counts[f]))
        np.testing.assert_array_equal(tr[f][0][-1], end[f][0])
        _same_trace(tr[f], tr2[f])


@pytest.mark.parametrize("dtype", [pyekf.EKF_F64, pyekf.EKF_F32], ids=["f64", "f32"])
def test_prefix_property(monkeypatch, dtype):
    """Record k − 1 of a 12-message device replay is, bit for bit, where a fresh handle given only
    the first k messages ends: a chunk's arithmetic does not depend on what follows it."""
    _env(monkeypatch)
    pyekf.poison_lds()
    arrs = _known_inputs(1, 12, 7, holes=False)
    tr, counts, _, st = _device_replay(96, 1, arrs, dtype=dtype)
    assert counts == [12] and st == [0]
    _moves(tr[0][0])
    for k in (1, 5, 12):
        _, ck, end, sk = _device_replay(96, 1, arrs, T=k, dtype=dtype)
        assert ck == [k] and sk == [0]
        np.testing.assert_array_equal(end[0][0], tr[0][0][k - 1])
        np.testing.assert_array_equal(end[0][1], tr[0][1][k - 1])


# ---- 4: association chunks ----

def _assoc_inputs(T=12, M=17, seed=23):
    sc = synth.synthetic(96, T, seed=seed, max_markers=M, shuffle=True)
    want = np.array([17, 16, 1, 0, -1, 17, 16, 17, 1, 0, 16, 17], np.int32)[:T]
    cnt = np.where(want > 0, np.minimum(want, sc.count), want).astype(np.int32)[:, None]
    return cnt, sc.rel[:, None], pyekf.odometry(sc)[:, None]


def _assoc_replay(cnt, rel, od, dtype, trace=True):
    e = pyekf.EKF(n_landmarks=96, dtype=dtype)
    assert e.path == pyekf.EKF_PATH_PIPELINE and e.assoc_route != pyekf.EKF_ASSOC_MARKER
    if trace:
        e.trace_enable(16)
    g = _gpu((cnt, rel, od))
    e.replay_device_assoc(*g)
    last = int(cnt[cnt[:, 0] > 0, 0][-1])
    out = dict(dec=e.decisions(last), state=e.state(), status=e.status(), route=e.assoc_route)
    if trace:
        out.update(count=e.trace_count(), trace=e.trace(), pose=e.pose(), tmo=e.map_odom())
    e.close()
    return out


@pytest.mark.parametrize("dtype", [pyekf.EKF_F64, pyekf.EKF_F32], ids=["f64", "f32"])
def test_association_chunks(monkeypatch, dtype):
    """N = 96 (two workgroups of k_assoc_msg a filter), m_max = 17 (two chunks a message), counts
    −1, 0, 1, 16 and 17: one record per message with count > 0, from the message's last chunk, by
    one workgroup; the same bits in either placement of the workgroups; the decisions as with the
    trace off; fp64 within 1e-8 of the oracle's sensor_cb, on the one-marker route too."""
    cnt, rel, od = _assoc_inputs()
    assert {-1, 0, 1, 16, 17} <= set(cnt[:, 0].tolist())
    active = int((cnt[:, 0] > 0).sum())
    _env(monkeypatch)
    pyekf.poison_lds()
    a = _assoc_replay(cnt, rel, od, dtype)
    assert a["status"] == 0 and a["count"] == active
    pose, tmo, seq = a["trace"]
    np.testing.assert_array_equal(seq, np.arange(active))
    np.testing.assert_array_equal(pose[-1], a["pose"])
    np.testing.assert_array_equal(tmo[-1], a["tmo"])
    _moves(pose)
    _env(monkeypatch, EKF_AM_XCD="0")
    b = _assoc_replay(cnt, rel, od, dtype)
    assert b["route"] == pyekf.EKF_ASSOC_CHUNK and b["count"] == active
    _same_trace(b["trace"], a["trace"])
    _env(monkeypatch)
    off = _assoc_replay(cnt, rel, od, dtype, trace=False)
    for x, y in zip(off["dec"], a["dec"]):
        np.testing.assert_array_equal(x, y)
    assert off["status"] == a["status"] and off["state"][2] == a["state"][2]
    np.testing.assert_array_equal(off["state"][0], a["state"][0])
    np.testing.assert_array_equal(off["state"][1], a["state"][1])
    if dtype != pyekf.EKF_F64:
        return
    po, to = _oracle_trace(96, np.clip(cnt[:, 0], 0, 17), rel[:, 0], od[:, 0])
    print("assoc chunks: max |pose - oracle|", np.abs(pose - po).max(), "max |tmo - oracle|",
          np.abs(tmo - to).max())
    assert np.abs(pose - po).max() < TOL and np.abs(tmo - to).max() < TOL
    # the one-marker route: k_assoc + a chain per marker, the chain writes the posterior
    _env(monkeypatch, EKF_ASSOC_MSG="0")
    e = pyekf.EKF(n_landmarks=96)
    assert e.assoc_route == pyekf.EKF_ASSOC_MARKER
    e.trace_enable(16)
    e.replay(np.clip(cnt, 0, 17), rel, od, assoc=True)
    assert e.trace_count() == active
    p1, t1, s1 = e.trace()
    np.testing.assert_array_equal(s1, np.arange(active))
    assert np.abs(p1 - po).max() < TOL and np.abs(t1 - to).max() < TOL
    np.testing.assert_array_equal(p1[-1], e.pose())
    e.close()


# ---- 5: capacity and lifecycle ----

def _raw_count(e, f=0):
    n = C.c_longlong(-5)
    return pyekf.lib().ekf_trace_count(e.h, f, C.byref(n)), n.value


def _raw_read(e, first, n, f=0):
    buf = (pyekf.TraceRec * max(n, 1))()
    got = C.c_int(-5)
    return pyekf.lib().ekf_trace_read(e.h, f, first, n, C.addressof(buf), C.byref(got)), got.value


def test_capacity_and_lifecycle(monkeypatch):
    _env(monkeypatch)
    pyekf.poison_lds()
    F, T = 2, 8
    arrs = _known_inputs(F, T + 2, 7, holes=False)
    cnt, ids, act, rel, od = arrs

    def feed(e, a, b):
        e.replay(cnt[a:b], rel[a:b], od[a:b], ids=ids[a:b], actions=act[a:b])

    small, twin = pyekf.EKF(n_landmarks=96, n_filters=F), pyekf.EKF(n_landmarks=96, n_filters=F)
    small.trace_enable(5)
    twin.trace_enable(16)
    feed(small, 0, T)
    feed(twin, 0, T)
    # beyond the capacity records are counted, not written
    assert small.trace_count() == T and twin.trace_count(1) == T
    ps, ts, ss = small.trace()
    assert len(ss) == 5
    _same_trace((ps, ts, ss), tuple(a[:5] for a in twin.trace()))
    assert _raw_read(small, 0, 9) == (pyekf.EKF_OK, 5)
    assert _raw_read(small, 3, 9) == (pyekf.EKF_OK, 2)
    assert _raw_read(small, 5, 1) == (pyekf.EKF_OK, 0)
    assert _raw_read(small, 7, 0) == (pyekf.EKF_OK, 0)
    assert _raw_read(small, -1, 1)[0] == pyekf.EKF_E_ARG
    assert _raw_read(small, 0, -1)[0] == pyekf.EKF_E_ARG
    assert _raw_count(small, F)[0] == pyekf.EKF_E_ARG and _raw_count(small, -1)[0] == pyekf.EKF_E_ARG
    assert pyekf.lib().ekf_trace_enable(small.h, -1) == pyekf.EKF_E_ARG
    assert small.trace_count() == T  # (a rejected call changed nothing)
    # the overflowing handle ends where its twin does
    for f in range(F):
        for x, y in zip(small.state(f), twin.state(f)):
            np.testing.assert_array_equal(x, y)
    # clear: the count and the next seq restart at 0
    small.trace_clear()
    assert [small.trace_count(f) for f in range(F)] == [0, 0]
    feed(small, T, T + 1)
    p, t, s = small.trace(1)
    assert s.tolist() == [0]
    np.testing.assert_array_equal(p[0], small.pose(1))
    # ekf_reset(f) restarts filter f's trace only
    twin.reset(1)
    assert [twin.trace_count(f) for f in range(F)] == [T, 0]
    twin.trace_clear(0)
    assert [twin.trace_count(f) for f in range(F)] == [0, 0]
    feed(twin, T, T + 2)
    assert [twin.trace(f)[2].tolist() for f in range(F)] == [[0, 1], [0, 1]]
    # enable(0) turns it off, and frees it
    twin.trace_enable(0)
    assert _raw_count(twin)[0] == pyekf.EKF_E_ARG
    assert pyekf.lib().ekf_trace_clear(twin.h, -1) == pyekf.EKF_E_ARG
    feed(twin, 0, 2)
    twin.sync()
    small.close()
    twin.close()


@pytest.mark.parametrize("N", [50, 96], ids=["resident", "pipeline"])
def test_trace_off_is_rejected_and_changes_nothing(monkeypatch, N):
    """A handle that never enabled the trace: count / read / clear return EKF_E_ARG, and after the
    same replay its state, Σ, counter and status equal the tracing twin's bit for bit."""
    _env(monkeypatch)
    pyekf.poison_lds()
    T = 10
    sc = synth.synthetic(N, T, seed=9, max_markers=12) if N == 96 else synth.basic_world(T)
    od = pyekf.odometry(sc)
    out = []
    for trace in (False, True):
        e = pyekf.EKF(n_landmarks=N)
        assert e.path == (pyekf.EKF_PATH_RESIDENT if N == 50 else pyekf.EKF_PATH_PIPELINE)
        if trace:
            e.trace_enable(4)  # (overflows: the count goes on alone)
        else:
            assert _raw_count(e) == (pyekf.EKF_E_ARG, -5)
            assert _raw_read(e, 0, 1) == (pyekf.EKF_E_ARG, -5)
            assert pyekf.lib().ekf_trace_clear(e.h, 0) == pyekf.EKF_E_ARG
        e.replay(sc.count[:, None], sc.rel[:, None], od[:, None], ids=sc.ids[:, None],
                 actions=sc.actions[:, None])
        e.posterior()
        out.append((e.state(), e.map_odom(), e.status()))
        if trace:
            assert e.trace_count() == T + 1
        e.close()
    (sa, ta, fa), (sb, tb, fb) = out
    assert fa == fb == 0 and sa[2] == sb[2]
    np.testing.assert_array_equal(sa[0], sb[0])
    np.testing.assert_array_equal(sa[1], sb[1])
    np.testing.assert_array_equal(ta, tb)


def test_enable_while_a_replay_is_in_flight(monkeypatch):
    """ekf_trace_enable synchronises: called right behind an asynchronous device replay it waits
    for it, and only what follows is recorded."""
    _env(monkeypatch)
    arrs = _known_inputs(1, 12, 7, holes=False)
    cnt, ids, act, rel, od = arrs
    ref, _, end, _ = _device_replay(96, 1, arrs)
    e = pyekf.EKF(n_landmarks=96)
    e.trace_enable(2)
    g = _gpu(tuple(a[:8] for a in arrs))
    e.replay_device(g[0], g[3], g[4], g[1], g[2])
    e.trace_enable(16)  # reallocates and clears, behind the replay
    g2 = _gpu(tuple(a[8:] for a in arrs))
    e.replay_device(g2[0], g2[3], g2[4], g2[1], g2[2])
    assert e.trace_count() == 4
    pose, tmo, seq = e.trace()
    assert seq.tolist() == [0, 1, 2, 3]
    np.testing.assert_array_equal(pose[-1], e.pose())
    # (the tail of the same drive replayed in one call, at the project's fp64 tolerance)
    assert np.abs(pose - ref[0][0][8:]).max() < TOL
    assert np.abs(tmo - ref[0][1][8:]).max() < TOL
    e.close()


# ---- 6: the per-call surface ----

def test_per_call_surface(monkeypatch):
    """Pipeline, N = 96: predict + correct + correct + posterior (k_posterior), fake_sensor (a
    chain) and sensor (k_assoc_msg) append one record each."""
    _env(monkeypatch)
    pyekf.poison_lds()
    sc = synth.synthetic(96, 3, seed=7, max_markers=4)
    od = pyekf.odometry(sc)
    e = pyekf.EKF(n_landmarks=96)
    e.trace_enable(8)
    e.set_odom(od[0])
    assert e.predict() == pyekf.EKF_OK
    for c in range(2):
        assert e.correct(sc.ids[0, c], *sc.rel[0, c]) == pyekf.EKF_OK
    assert e.trace_count() == 0  # (corrections alone store no posterior)
    assert e.posterior() == pyekf.EKF_OK
    assert e.trace_count() == 1
    np.testing.assert_array_equal(e.trace()[0][0], e.pose())
    np.testing.assert_array_equal(e.trace()[1][0], e.map_odom())
    e.set_odom(od[1])
    c = int(sc.count[1])
    assert e.fake_sensor(sc.ids[1, :c], sc.actions[1, :c], sc.rel[1, :c]) == pyekf.EKF_OK
    assert e.trace_count() == 2
    e.set_odom(od[2])
    c = int(sc.count[2])
    assert e.sensor(sc.rel[2, :c])[0] == pyekf.EKF_OK
    assert e.trace_count() == 3
    pose, tmo, seq = e.trace()
    assert seq.tolist() == [0, 1, 2]
    _moves(pose)
    np.testing.assert_array_equal(pose[-1], e.pose())
    np.testing.assert_array_equal(tmo[-1], e.map_odom())
    assert e.status() == 0
    e.close()


# ---- 7: the simulator forms ----

def _sim_for(e, sw, **kw):
    return pyekf.Sim(e, sw.landmarks, seed=int(sw.seeds[0]), ticks_per_msg=sw.wheel.shape[1],
                     max_markers=min(16, sw.landmarks.shape[1]), marker_stride=sw.ids.shape[2],
                     start_theta=sw.start_pose[0], start_x=sw.start_pose[1],
                     start_y=sw.start_pose[2], record=1, **kw)


@pytest.mark.parametrize("form", ["pipeline_parallel", "resident"])
def test_simulator_forms(monkeypatch, form):
    """ekf_sim_run, T = 8: the parallel form on a pipeline handle (N = 96, F = 3: planned by
    ekf_replay_device's planner) and k_sim's in-place descriptors on a resident one (N = 50)."""
    _env(monkeypatch)
    pyekf.poison_lds()
    F, T = 3, 8
    if form == "resident":
        drive = synth.circle_drive(T, 0.3, sense=synth.SENSE_ALL)
        seeds = np.uint64(777) + np.arange(F, dtype=np.uint64)
        sw = synth._generate(50, drive, seeds, synth.BASIC_WORLD_LANDMARKS,
                             start_pose=(synth.BASIC_WORLD_THETA0, 0.0, 0.0), max_range=0.8)
        e = pyekf.EKF(n_landmarks=50, n_filters=F)
        assert e.path == pyekf.EKF_PATH_RESIDENT
        sim = _sim_for(e, sw, max_range=0.8)
    else:
        sw = synth.swarm(96, F, T, survey=False)
        e = pyekf.EKF(n_landmarks=96, n_filters=F)
        assert e.path == pyekf.EKF_PATH_PIPELINE
        sim = _sim_for(e, sw)
    e.trace_enable(T)
    sim.run(sw.cmd, sw.sense)
    cnt = sim.markers()[0]
    assert cnt.shape == (T, F)
    for f in range(F):
        k = int((cnt[:, f] >= 1).sum())
        assert k >= 2
        assert e.trace_count(f) == k
        pose, tmo, seq = e.trace(f)
        np.testing.assert_array_equal(seq, np.arange(k))
        _moves(pose)
        np.testing.assert_array_equal(pose[-1], e.pose(f))
        np.testing.assert_array_equal(tmo[-1], e.map_odom(f))
        assert e.status(f) == 0
    sim.close()
    e.close()


# ---- 8: slam_replay_trace ----

def test_slam_replay_trace(monkeypatch):
    """The node mirror, N = 50, unknown association, the first 40 scans of synth.lidar_world through
    the front-end: slam_replay_trace's rows equal slam_replay's per-message read-backs within 1e-8,
    the rows of scans without markers included, from ONE resident launch."""
    from pyekf.landmarks import Detector
    _env(monkeypatch)
    pyekf.poison_lds()
    sc, _, scans = synth.lidar_world()
    T = 40
    scans = scans[:T]
    inc = float(np.float32(2 * math.pi / 360))
    det = Detector(max_scans=T, max_beams=360)
    cnt, mk = det.detect(scans, np.zeros(T), np.full(T, inc))
    det.close()
    c = np.clip(cnt, 0, mk.shape[1])
    c[7] = 0   # two scans without markers: their rows repeat the row before
    c[21] = 0
    keep = np.arange(mk.shape[1])[None, :] < c[:, None]
    rel = np.stack([np.where(keep, mk["x"], 0.0), np.where(keep, mk["y"], 0.0)], -1)
    scg = synth.Scenario(sc.n_landmarks, sc.landmarks, sc.wheel[:T],
                         np.full(keep.shape, -1, np.int32), np.zeros(keep.shape, np.int32), rel,
                         c.astype(np.int32), sc.truth[:T], sc.track, sc.radius)
    assert (c > 0).sum() >= 30
    a, b = (pyekf.Slam(n_landmarks=50, source=pyekf.SOURCE_ASSOC) for _ in range(2))
    assert a.path == pyekf.EKF_PATH_RESIDENT
    rc_b, pose_b, tmo_b = b.replay(scg, poses=True)
    a.profile(True)
    rc_a, pose_a, tmo_a = a.replay(scg, poses=True, trace=True)
    assert a.profile_read(4)[0] == 1  # the point of the feature
    assert rc_a == rc_b == pyekf.EKF_E_EMPTY  # (the first non-OK status: the empty MarkerArrays)
    assert np.ptp(pose_b[:, 1:], axis=0).max() > 0.1  # (the robot drives)
    print("slam_replay_trace: max |pose - slam_replay|", np.abs(pose_a - pose_b).max(),
          "max |tmo - slam_replay|", np.abs(tmo_a - tmo_b).max())
    assert np.abs(pose_a - pose_b).max() < TOL
    assert np.abs(tmo_a - tmo_b).max() < TOL
    for t in (7, 21):
        np.testing.assert_array_equal(pose_a[t], pose_a[t - 1])
        np.testing.assert_array_equal(tmo_a[t], tmo_a[t - 1])
    (xa, Sa, ca), (xb, Sb, cb) = a.filter_state(), b.filter_state()
    assert ca == cb and np.abs(xa - xb).max() < TOL and np.abs(Sa - Sb).max() < TOL
    # a second drive on the same node: the trace is cleared first, row −1 is where the first ended
    rc2, pose2, _ = a.replay(scg, poses=True, trace=True)
    assert pose2.shape == (T, 3) and np.isfinite(pose2).all()
    a.close()
    b.close()
