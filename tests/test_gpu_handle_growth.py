"""The handles' grown-on-demand buffers (ekf-slam_amd/csrc/hip_owned.hpp) on the GPU: a handle
driven across a regrowth of one of its buffers ends byte-equal to a fresh handle that got the same
inputs without regrowing.

State means state() (x, Σ, counter), map_odom() and status(), compared as bytes: growth keeps no
contents and moves nothing a kernel reads in flight, so nothing may differ, not by one bit. (What a
failed allocation leaves behind cannot be provoked here: tests/test_hip_owned_host.py runs those
paths on the CPU.)"""
import numpy as np
import pytest

import pyekf
from pyekf import synth

pytestmark = pytest.mark.gpu

ENV = ("EKF_SERIAL", "EKF_CU_SPLIT", "EKF_DEVSYNC", "EKF_AM_XCD", "EKF_ASSOC_MSG", "EKF_STAGE",
       "EKF_RESIDENT", "EKF_SIM_PARALLEL", "EKF_CHAIN_FAST")
DESC_INIT = 256   # kDescInit (ekf_ctx.hpp): descriptors a handle of ≤ 64 filters starts with


def _env(monkeypatch, **kv):
    for k in ENV:
        monkeypatch.delenv(k, raising=False)
    for k, v in kv.items():
        monkeypatch.setenv(k, v)


def _gpu(*arrs):
    import torch
    return [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in arrs]


def _snap(e):
    """Every filter's state, as bytes and exact integers."""
    out = []
    for f in range(e.F):
        x, S, c = e.state(f)
        out.append((x.tobytes(), S.tobytes(), c, e.map_odom(f).tobytes(), e.status(f)))
    return out


def _messages(N, F, T, M, shuffle, seed0):
    """Filter f = its own map and drive: counts [T,F], ids / actions [T,F,M], rel [T,F,M,2] (padded
    with empty markers up to M), odom [T,F,3]."""
    cnt, ids = np.zeros((T, F), np.int32), np.full((T, F, M), -1, np.int32)
    act, rel, od = np.zeros((T, F, M), np.int32), np.zeros((T, F, M, 2)), np.zeros((T, F, 3))
    for f in range(F):
        sc = synth.make_scenario(N, synth.random_landmarks(N, seed=seed0 + f), T, max_markers=M,
                                 seed=seed0 + 50 + f, shuffle=shuffle)
        m = sc.ids.shape[1]
        cnt[:, f], ids[:, f, :m], act[:, f, :m] = sc.count, sc.ids, sc.actions
        rel[:, f, :m], od[:, f] = sc.rel, pyekf.odometry(sc)
    assert (cnt > 0).all()
    return cnt, ids, act, rel, od


# ---- 1: the descriptor buffer ----

@pytest.mark.parametrize("kind", ["known", "assoc"])
def test_descriptor_buffer_regrowth(monkeypatch, kind):
    """A pipeline handle, fp64, N = 4, F = 2. known: ekf_replay_device of T = 160 messages of one
    marker, T·F = 320 descriptors > kDescInit, against two replays of 80. assoc:
    ekf_replay_device_assoc of T = 80 messages of m_max = 17 (two chunks each: 320 descriptors)
    against four replays of 20."""
    _env(monkeypatch, EKF_RESIDENT="0")
    N, F = 4, 2
    assoc = kind == "assoc"
    T, M, parts = (80, 17, 4) if assoc else (160, 1, 2)
    C = (M + 15) // 16
    assert T * C * F > DESC_INIT >= T // parts * C * F
    cnt, ids, act, rel, od = _messages(N, F, T, M, assoc, 700 if assoc else 600)

    def drive(e, bounds):
        keep = []
        for a, b in zip(bounds[:-1], bounds[1:]):
            g = _gpu(cnt[a:b], rel[a:b], od[a:b], ids[a:b], act[a:b])
            keep.append(g)
            if assoc:
                e.replay_device_assoc(g[0], g[1], g[2])
            else:
                e.replay_device(*g)
        e.sync()   # (the tensors may go once the replays have read them)
        return _snap(e)

    grown = pyekf.EKF(n_landmarks=N, n_filters=F)
    assert grown.path == pyekf.EKF_PATH_PIPELINE
    if assoc and grown.assoc_route == pyekf.EKF_ASSOC_MARKER:
        grown.close()
        pytest.skip("no device-planned association replay on the one-marker route")
    fresh = pyekf.EKF(n_landmarks=N, n_filters=F)
    got = drive(grown, [0, T])
    want = drive(fresh, list(range(0, T + 1, T // parts)))
    assert all(np.frombuffer(s[0]).any() for s in want)   # (the replays ran)
    assert got == want
    grown.close()
    fresh.close()


# ---- 2: the three scoring entry points through one buffer ----

def test_scoring_calls_share_one_buffer(monkeypatch):
    """A resident handle, N = 4, F = 3, after a 5-message known-id replay: marginals(f = 0), eval
    with n_map = 4, eval_match with n_map = 9 (each a larger buffer than the one before), then
    marginals of every filter in the buffer as it is by then. Each result equals the same call
    made first on a fresh, identically driven handle."""
    _env(monkeypatch)
    N, F, T = 4, 3, 5
    cnt, ids, act, rel, od = _messages(N, F, T, 4, False, 800)
    rng = np.random.default_rng(5)
    truth_pose = rng.normal(size=(F, 3))
    truth4 = rng.uniform(-2, 2, size=(F, 4, 2))
    truth9 = rng.uniform(-2, 2, size=(F, 9, 2))

    def handle():
        e = pyekf.EKF(n_landmarks=N, n_filters=F)
        assert e.path == pyekf.EKF_PATH_RESIDENT
        e.replay(cnt, rel, od, ids=ids, actions=act)
        return e

    calls = [lambda e: e.marginals(f=0),
             lambda e: e.eval(truth_pose, truth4),
             lambda e: e.eval_match(truth_pose, truth9, 0.5),
             lambda e: e.marginals(f=None)]

    def as_bytes(res):
        return [np.asarray(r).tobytes() for r in (res if isinstance(res, tuple) else (res,))]

    one = handle()
    got = [as_bytes(call(one)) for call in calls]
    state = _snap(one)
    one.close()
    for k, call in enumerate(calls):
        e = handle()
        assert as_bytes(call(e)) == got[k], k
        assert _snap(e) == state       # (scoring reads only)
        e.close()
    assert len(set(map(tuple, got))) == len(got)


# ---- 3: the trace re-allocated ----

def test_trace_reallocation(monkeypatch):
    """trace_enable(2), 5 messages, trace_enable(8), 5 messages, trace_enable(0), trace_enable(8):
    5 appended (2 kept), 5 appended (5 kept), off (EKF_E_ARG), 0; the state an untraced handle's
    throughout."""
    _env(monkeypatch)
    N, F = 4, 1
    cnt, ids, act, rel, od = _messages(N, F, 10, 4, False, 900)
    traced, plain = (pyekf.EKF(n_landmarks=N, n_filters=F) for _ in range(2))

    def run(a, b):
        for e in (traced, plain):
            e.replay(cnt[a:b], rel[a:b], od[a:b], ids=ids[a:b], actions=act[a:b])
        assert _snap(traced) == _snap(plain)

    traced.trace_enable(2)
    run(0, 5)
    assert traced.trace_count() == 5 and len(traced.trace()[2]) == 2
    traced.trace_enable(8)
    assert traced.trace_count() == 0
    run(5, 10)
    assert traced.trace_count() == 5
    pose, _, seq = traced.trace()
    assert seq.tolist() == [0, 1, 2, 3, 4]
    assert pose[-1].tobytes() == plain.pose().tobytes()
    traced.trace_enable(0)
    with pytest.raises(pyekf.EkfError) as err:
        traced.trace_count()
    assert err.value.rc == pyekf.EKF_E_ARG
    traced.trace_enable(8)
    assert traced.trace_count() == 0 and len(traced.trace()[2]) == 0
    assert _snap(traced) == _snap(plain)
    traced.close()
    plain.close()


# ---- 4: create, use every lazy allocation, destroy ----

def test_create_use_destroy_rounds(monkeypatch):
    """Eight rounds in one process on a pipeline handle, N = 8, F = 2, marker_stride = 16: the
    trace, Sim.run and Sim.run_assoc with T growing 2, 3, 4, 5 (the simulator's run buffers regrow
    every time; the planning state and the association scratch at their first use), a device
    replay, a host-planned association chunk, both evals. Every round ends as round 1 did."""
    _env(monkeypatch, EKF_RESIDENT="0")
    N, F, T = 8, 2, 20
    sw = synth.swarm(N, F, T, survey=False, marker_stride=16)
    assert sw.ids.shape[2] == 16
    tpm = sw.wheel.shape[1]
    od = np.repeat(pyekf.odometry(sw.scenario(0))[:, None], F, 1)
    start = np.array(sw.start_pose, np.float64)
    first = None
    for rnd in range(8):
        e = pyekf.EKF(n_landmarks=N, n_filters=F)
        assert e.path == pyekf.EKF_PATH_PIPELINE
        if e.assoc_route == pyekf.EKF_ASSOC_MARKER:
            e.close()
            pytest.skip("Sim.run_assoc needs a chunk route: none on the one-marker route")
        e.trace_enable(4)
        sim = pyekf.Sim(e, sw.landmarks, seed=int(sw.seeds[0]), ticks_per_msg=tpm, max_markers=N,
                        marker_stride=16, start_theta=start[0], start_x=start[1],
                        start_y=start[2], record=1)
        t = 0
        for n, run in ((2, sim.run), (3, sim.run), (4, sim.run_assoc), (5, sim.run_assoc)):
            run(sw.cmd[t * tpm:(t + n) * tpm])
            t += n
        scored = sim.eval().tobytes()
        a, b = t, t + 3
        g = _gpu(sw.count[a:b], sw.rel[a:b], od[a:b], sw.ids[a:b], sw.actions[a:b])
        e.replay_device(*g)
        e.sync()
        a, b = b, T
        e.replay(sw.count[a:b], sw.rel[a:b], od[a:b], ids=None, assoc=True)
        end = (_snap(e), scored, e.eval(sw.truth[T - 1], sw.landmarks, frame=start).tobytes(),
               [e.trace_count(f) for f in range(F)])
        sim.close()
        e.close()
        if first is None:
            first = end
            assert all(n == T for n in end[3])
        assert end == first, rnd
