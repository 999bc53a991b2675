"""ekf_sim_fork on the GPU: a forked swarm continues the source filter's run.

Source and destination simulators share seed and f0 over handles of three filters, the basic
world's four landmarks, record on. The source runs three messages (a SURVEY among them, two
markers a message, so its sighted set is neither empty nor full), filter 1 is forked into the
destination, and both run the same three further messages. Destination filter 1 then has source
filter 1's state, seed and draw indices, so it must equal it bit for bit in everything the
simulator and the filter report; filters 0 and 2 start from the same state under their own seeds.
"""
import functools

import numpy as np
import pytest

import pyekf
from pyekf import synth

pytestmark = pytest.mark.gpu

F, T1, T2, SRC = 3, 3, 3, 1
START = (synth.BASIC_WORLD_THETA0, 0.0, 0.0)
SENSE1 = np.array([synth.SENSE_NEAREST, synth.SENSE_SURVEY, synth.SENSE_NEAREST], np.int32)
SENSE2 = np.array([synth.SENSE_SURVEY, synth.SENSE_NEAREST, synth.SENSE_SURVEY], np.int32)
CONFIG = dict(seed=4242, f0=5, max_markers=2, marker_stride=4, max_range=1.5, record=1,
              start_theta=START[0], start_x=START[1], start_y=START[2])


@functools.lru_cache(maxsize=None)
def _cmd():
    """Commanded wheel increments per tick of a 0.3 m circle, T1 + T2 messages of 40 ticks."""
    drive = synth.circle_drive(T1 + T2, 0.3)
    sw = synth._generate(50, drive, [1], synth.BASIC_WORLD_LANDMARKS, start_pose=START)
    return sw.cmd


def _pair(monkeypatch, pipeline, N=50, collide=False, **cfg):
    if pipeline:
        monkeypatch.setenv("EKF_RESIDENT", "0")
    else:
        monkeypatch.delenv("EKF_RESIDENT", raising=False)
    e = pyekf.EKF(N, F)
    assert e.path == (pyekf.EKF_PATH_PIPELINE if pipeline else pyekf.EKF_PATH_RESIDENT)
    sim = pyekf.Sim(e, synth.BASIC_WORLD_LANDMARKS, **dict(CONFIG, **cfg))
    if collide:
        sim.set_collisions(0.11, 0.038)
    return e, sim


def _snap(e, f):
    x, S, cnt = e.state(f)
    return x, S, cnt, e.map_odom(f)


def _same_filter(a, b):
    for u, v in zip(a[:2] + a[3:], b[:2] + b[3:]):
        np.testing.assert_array_equal(u, v)
    assert a[2] == b[2]


def _first(sim, e, run=None):
    tpm = sim.cfg.ticks_per_msg
    (run or sim.run)(_cmd()[:T1 * tpm], SENSE1)
    e.sync()


@pytest.mark.parametrize("case", ["resident", "pipeline", "pipeline-parallel", "collisions",
                                  "assoc"])
def test_a_fork_continues_the_run(monkeypatch, case):
    pipeline = case in ("pipeline", "pipeline-parallel", "assoc")
    collide = case == "collisions"
    e1, s1 = _pair(monkeypatch, pipeline, collide=collide)
    e2, s2 = _pair(monkeypatch, pipeline, collide=collide)
    _first(s1, e1)
    assert e1.state(SRC, sigma=False)[0][3:].any()  # (landmarks mapped)
    s2.fork_from(s1, SRC)
    want = s1.eval()[SRC].tobytes()
    for f in range(F):  # every destination filter starts from the source filter's state,
        _same_filter(_snap(e2, f), _snap(e1, SRC))
        assert s2.eval()[f].tobytes() == want  # ... true pose and map
    cmd = _cmd()[T1 * s1.cfg.ticks_per_msg:]
    for s in (s1, s2):
        if case == "assoc":
            s.run_assoc(cmd)
        else:
            s.run(cmd, None if case == "pipeline-parallel" else SENSE2)
    m1, m2 = s1.markers(), s2.markers()
    for a, b in zip(m1, m2):  # counts, ids, actions, rel of the run after the fork
        assert a.shape[0] == T2
        np.testing.assert_array_equal(a[:, SRC], b[:, SRC])
    (o1, t1), (o2, t2) = s1.poses(), s2.poses()
    np.testing.assert_array_equal(o1, o2)
    np.testing.assert_array_equal(t1[:, SRC], t2[:, SRC])
    _same_filter(_snap(e2, SRC), _snap(e1, SRC))
    r1, r2 = s1.eval(), s2.eval()
    assert r1[SRC].tobytes() == r2[SRC].tobytes()
    for f in (0, 2):  # their own seeds: other noise on the markers, a sound run
        assert not np.array_equal(m2[3][:, f], m2[3][:, SRC])
        assert not np.array_equal(t2[:, f], t2[:, SRC])
        assert np.isfinite(r2[f]["pose_err"]).all() and np.isfinite(r2[f]["pose_nees"])
        assert np.isfinite(r2[f]["lm_sq_err"]) and r2[f]["n_seen"] > 0
        assert e2.status(f) == 0
    assert e1.status(SRC) == e2.status(SRC) == 0
    for o in (s1, s2, e1, e2):
        o.close()


@pytest.mark.parametrize("pipeline", [False, True], ids=["resident", "pipeline"])
def test_fork_inside_one_simulator(monkeypatch, pipeline):
    e, s = _pair(monkeypatch, pipeline)
    ref_e, ref_s = _pair(monkeypatch, pipeline)
    _first(s, e)
    _first(ref_s, ref_e)
    own, rec = _snap(e, SRC), s.eval()
    assert rec[0].tobytes() != rec[SRC].tobytes() != rec[2].tobytes()
    s.fork_from(s, SRC)
    _same_filter(_snap(e, SRC), own)
    for f in range(F):  # (the record: the filter against the simulator's true pose and map)
        _same_filter(_snap(e, f), own)
        assert s.eval()[f].tobytes() == rec[SRC].tobytes()
    # the source filter goes on as in a simulator that never forked; the others from its poses
    cmd = _cmd()[T1 * s.cfg.ticks_per_msg:]
    s.run(cmd, SENSE2)
    ref_s.run(cmd, SENSE2)
    _same_filter(_snap(e, SRC), _snap(ref_e, SRC))
    for a, b in zip(s.markers(), ref_s.markers()):
        np.testing.assert_array_equal(a[:, SRC], b[:, SRC])
    t, rt = s.poses()[1], ref_s.poses()[1]
    np.testing.assert_array_equal(t[:, SRC], rt[:, SRC])
    for f in (0, 2):
        assert not np.array_equal(t[:, f], t[:, SRC])
    assert np.isfinite(s.eval()["pose_nees"]).all()
    for o in (s, ref_s, e, ref_e):
        o.close()


def test_errors_change_nothing_and_move_no_counter(monkeypatch):
    L, E = pyekf.lib(), pyekf.EKF_E_ARG
    e1, s1 = _pair(monkeypatch, False)
    _first(s1, e1)
    e2, s2 = _pair(monkeypatch, False)
    tpm = s2.cfg.ticks_per_msg
    s2.run(_cmd()[:tpm], SENSE1[:1])
    e2.sync()
    before = [_snap(e2, f) for f in range(F)]
    # what the source would have to agree on
    e3, s3 = _pair(monkeypatch, False, ticks_per_msg=20)
    e4, s4 = _pair(monkeypatch, False, start_x=0.25)
    e5 = pyekf.EKF(50, F)
    s5 = pyekf.Sim(e5, synth.BASIC_WORLD_LANDMARKS[:3], **CONFIG)
    e6, s6 = _pair(monkeypatch, False, N=8)  # a smaller destination map
    assert L.ekf_sim_fork(s2.h, s3.h, SRC) == E
    assert L.ekf_sim_fork(s2.h, s4.h, SRC) == E
    assert L.ekf_sim_fork(s2.h, s5.h, SRC) == E
    assert L.ekf_sim_fork(s2.h, s1.h, F) == E
    assert L.ekf_sim_fork(s2.h, s1.h, -1) == E
    assert L.ekf_sim_fork(s6.h, s1.h, SRC) == E
    assert L.ekf_sim_fork(None, s1.h, SRC) == E
    assert L.ekf_sim_fork(s2.h, None, SRC) == E
    for f in range(F):
        _same_filter(_snap(e2, f), before[f])
    # no counter moved: the next message draws what it draws in a simulator nobody tried to fork
    e7, s7 = _pair(monkeypatch, False)
    s7.run(_cmd()[:tpm], SENSE1[:1])
    for s in (s2, s7):
        s.run(_cmd()[tpm:2 * tpm], SENSE1[1:2])
    for a, b in zip(s2.markers(), s7.markers()):
        np.testing.assert_array_equal(a, b)
    np.testing.assert_array_equal(s2.poses()[1], s7.poses()[1])
    for f in range(F):
        _same_filter(_snap(e2, f), _snap(e7, f))
    for o in (s1, s2, s3, s4, s5, s6, s7, e1, e2, e3, e4, e5, e6, e7):
        o.close()
