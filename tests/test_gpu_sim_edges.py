"""The on-device simulator (ekf-slam_amd/csrc/sim_kernels.hip: k_sim, k_sim_arcs, k_sim_pose,
k_sim_sense) at the edges of its parameter space, on the cases of tests/sim_cases.py (pinned on the
CPU by tests/test_sim_cases.py: each reaches its path and is decidable at GAP = 1e-6).

Per case and form:
* inputs against pyekf.synth after every run: counts, ids and actions exactly, rel, truth and
  odometry within SIM_TOL = 1e-9 (tests/test_gpu_sim.py), the padding from count to the stride
  exactly −1 / 0 / 0.0;
* forms against each other: where the parallel form may run, the recorded markers and poses of
  EKF_SIM_PARALLEL=1, EKF_SIM_PARALLEL=0 and (empty, empty-tail) ekf_sim_run_assoc are the same
  bytes;
* the filter: status 0; a twin handle fed the run's own recorded arrays run by run through
  replay_on_device ends byte-identical where the run used that entry point (the parallel form,
  run_assoc on both paths); the sequential form against ekf_replay planned on the host at
  test_sim_schedules_and_host_replay_agree's 1e-9 (state) and 1e-8 (Σ); the C oracle fed the
  device's markers for N ≤ 128 (the dense oracle at N = 1024 takes too long here), a message with
  no marker giving it set_odom alone, as ekf_replay with a count of 0.

Oracle bounds, inherited from tests/test_gpu_sim.py, none measured anew: POSE_TOL = 1e-8 on the
basic world (all-delete), STATE_TOL_POPULATED = 5e-8 and SIGMA_TOL = 1e-7 on the random maps, whose
chunks fold first sightings (the 1e7 prior) and corrections into one factored update as the survey
maps' do (that file's docstring).
"""
import numpy as np
import pytest

import orc
import pyekf
from pyekf import synth

import sim_cases as sc
import test_gpu_eval as tge
from test_gpu_sim import POSE_TOL, SIGMA_TOL, SIM_TOL, STATE_TOL_POPULATED

pytestmark = pytest.mark.gpu

HOST_STATE_TOL, HOST_SIGMA_TOL = 1e-9, 1e-8   # test_sim_schedules_and_host_replay_agree
ORACLE_MAX_N = 128

PIPELINE_CASES = [n for n in sc.NAMES if not n.endswith("-small")]
RESIDENT_CASES = ["empty", "mixed-all", "all-delete", "ticks-64-small", "markers-1-small"]


# ---- test_gpu_sim.py's helpers, with the case's keywords, the padding and the empty messages ------
def _sim_for(e, case, **over):
    return pyekf.Sim(e, case.sw.landmarks, **{**case.sim_kw, **over})


def _check_inputs(sim, sw, t0=0):
    cnt, ids, act, rel = sim.markers()
    odom, truth = sim.poses()
    T = cnt.shape[0]
    sl = slice(t0, t0 + T)
    assert ids.shape == sw.ids[sl].shape
    print(f"  messages [{t0}, {t0 + T}): truth {np.abs(truth - sw.truth[sl]).max():.3g}, odom "
          f"{np.abs(odom - pyekf.odometry(sw.scenario(0))[sl]).max():.3g}, rel "
          f"{np.abs(rel - sw.rel[sl]).max():.3g}")
    assert np.abs(truth - sw.truth[sl]).max() < SIM_TOL
    assert np.abs(odom - pyekf.odometry(sw.scenario(0))[sl]).max() < SIM_TOL
    np.testing.assert_array_equal(cnt, sw.count[sl])
    np.testing.assert_array_equal(ids, sw.ids[sl])
    np.testing.assert_array_equal(act, sw.actions[sl])
    assert np.abs(rel - sw.rel[sl]).max() < SIM_TOL
    pad = np.arange(ids.shape[2])[None, None, :] >= cnt[..., None]
    assert (ids[pad] == -1).all() and (act[pad] == 0).all()
    assert (rel[pad].view(np.uint64) == 0).all()      # +0.0, not −0.0
    return cnt, ids, act, rel, odom, truth


def _runs(sim, case, assoc=False):
    """Every run of the case; the inputs checked after each. Returns the runs' recorded arrays."""
    sw, tpm = case.sw, case.sw.wheel.shape[1]
    parts = []
    for a, b in case.bounds:
        if assoc:
            sim.run_assoc(sw.cmd[a * tpm:b * tpm])
        else:
            sim.run(sw.cmd[a * tpm:b * tpm], sw.sense[a:b])
        parts.append(_check_inputs(sim, sw, a))
    return parts


def _cat(parts):
    return [np.concatenate(p) for p in zip(*parts)]


def _bytes(parts):
    return [a.tobytes() for p in parts for a in p]


def _oracle(N, cnt, ids, act, rel, odom, f, joseph=False):
    ref = orc.OracleEKF(n_landmarks=N, joseph=joseph)
    for t in range(cnt.shape[0]):
        ref.set_odom(odom[t])
        c = int(cnt[t, f])
        if c:
            ref.fake_sensor_cb(ids[t, f, :c], act[t, f, :c], rel[t, f, :c])
    return ref.get()


def _states(e):
    out = [e.state(f) for f in range(e.F)]
    assert [e.status(f) for f in range(e.F)] == [0] * e.F
    return out


def _twin(case, N, parts, known, joseph=False, trace=0):
    """A second handle fed the runs' recorded arrays, run by run, by the replay underneath."""
    e2 = pyekf.EKF(n_landmarks=N, n_filters=case.sw.n_filters)
    if joseph:
        assert e2.set_joseph(True) == pyekf.EKF_OK
    if trace:
        e2.trace_enable(trace)
    for cnt, ids, act, rel, odom, _ in parts:
        dev = tge._gpu((cnt, rel, np.repeat(odom[:, None], cnt.shape[1], 1), ids, act))
        if known:
            e2.replay_on_device(dev[0], dev[1], dev[2], ids=dev[3], actions=dev[4])
        else:
            e2.replay_on_device(dev[0], dev[1], dev[2], ids=None)
        e2.sync()        # (the tensors may go once the replay has read them)
    return e2


def _against_host_replay(case, N, parts, got, joseph=False):
    cnt, ids, act, rel, odom, _ = _cat(parts)
    w = max(1, int(cnt.max()))
    e = pyekf.EKF(n_landmarks=N, n_filters=cnt.shape[1])
    if joseph:
        assert e.set_joseph(True) == pyekf.EKF_OK
    e.replay(cnt, rel[:, :, :w], np.repeat(odom[:, None], cnt.shape[1], 1), ids=ids[:, :, :w],
             actions=act[:, :, :w])
    for f, (x, S, c) in enumerate(_states(e)):
        dx, dS = np.abs(x - got[f][0]).max(), np.abs(S - got[f][1]).max()
        print(f"  filter {f} against the host-planned replay: state {dx:.3g}, sigma {dS:.3g}")
        assert c == got[f][2]
        assert dx < HOST_STATE_TOL and dS < HOST_SIGMA_TOL, f
    e.close()


def _against_oracle(case, N, parts, got, joseph=False):
    if N > ORACLE_MAX_N:
        return
    cnt, ids, act, rel, odom, _ = _cat(parts)
    tol_x, tol_S = (POSE_TOL, POSE_TOL) if case.basic_world else (STATE_TOL_POPULATED, SIGMA_TOL)
    for f in sorted({0, cnt.shape[1] - 1}):
        xr, Sr, _, cr = _oracle(N, cnt, ids, act, rel, odom, f, joseph)
        x, S, c = got[f]
        dx, dS = np.abs(x - xr).max(), np.abs(S - Sr).max()
        print(f"  filter {f} against the oracle: state {dx:.3g}, sigma {dS:.3g}")
        assert c == cr
        assert dx < tol_x and dS < tol_S, f


def _run_form(case, N, path, joseph=False):
    """One known-id form of the case on a fresh handle: inputs, status, the form's filter checks.
    Returns (recorded parts, states)."""
    e = pyekf.EKF(n_landmarks=N, n_filters=case.sw.n_filters)
    assert e.path == path
    if joseph:
        assert e.set_joseph(True) == pyekf.EKF_OK
    sim = _sim_for(e, case)
    parts = _runs(sim, case)
    got = _states(e)
    sim.close()
    e.close()
    return parts, got


# ---- the pipeline, both forms --------------------------------------------------------------------
@pytest.mark.parametrize("name", PIPELINE_CASES)
def test_case_on_the_pipeline_in_both_forms(name, monkeypatch):
    pyekf.poison_lds()
    case = sc.get(name)
    N = case.n_slots
    monkeypatch.setenv("EKF_RESIDENT", "0")
    runs = {}
    for env in ("1", "0"):
        print(f"{name}, EKF_SIM_PARALLEL={env}")
        monkeypatch.setenv("EKF_SIM_PARALLEL", env)
        parts, got = _run_form(case, N, pyekf.EKF_PATH_PIPELINE)
        runs[env] = parts
        if env == "1" and case.parallel:
            # the parallel form is ekf_replay_device over the recorded arrays: the same bytes
            e2 = _twin(case, N, parts, known=True)
            for (x, S, c), (x2, S2, c2) in zip(got, _states(e2)):
                assert x.tobytes() == x2.tobytes() and S.tobytes() == S2.tobytes() and c == c2
            e2.close()
        else:
            _against_host_replay(case, N, parts, got)
        _against_oracle(case, N, parts, got)
    # (a case with a SURVEY message or a stride beyond a chunk ran k_sim twice: the same bytes too)
    assert _bytes(runs["1"]) == _bytes(runs["0"])


# ---- the resident path ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", RESIDENT_CASES)
def test_case_on_the_resident_path(name):
    pyekf.poison_lds()
    case = sc.get(name)
    N = case.n_slots
    assert N <= 62
    parts, got = _run_form(case, N, pyekf.EKF_PATH_RESIDENT)
    _against_host_replay(case, N, parts, got)
    _against_oracle(case, N, parts, got)


# ---- unknown association over messages with no marker ---------------------------------------------
@pytest.mark.parametrize("N,path", [(96, pyekf.EKF_PATH_PIPELINE), (40, pyekf.EKF_PATH_RESIDENT)],
                         ids=["pipeline96", "resident40"])
@pytest.mark.parametrize("name", ["empty", "empty-tail"])
def test_run_assoc_over_empty_messages(name, N, path, monkeypatch):
    """Twin and byte comparisons only: with holes in the stream the association's decision margins
    against the oracle are not established."""
    pyekf.poison_lds()
    case = sc.get(name)
    assert (case.sw.count == 0).any() and case.nearest_only
    F = case.sw.n_filters
    e = pyekf.EKF(n_landmarks=N, n_filters=F)
    assert e.path == path
    e.trace_enable(32)
    sim = _sim_for(e, case)
    parts = _runs(sim, case, assoc=True)
    e2 = _twin(case, N, parts, known=False, trace=32)
    m = case.stride
    # a filter takes a record per message that has a marker for it, and none for the others
    assert [e.trace_count(f) for f in range(F)] == (case.sw.count > 0).sum(0).tolist()
    ra, sa = tge._everything(e, m)
    rb, sb = tge._everything(e2, m)
    assert ra == rb and sa == sb
    # the markers and poses are those of the known-id forms, bit for bit
    for env in ("1", "0"):
        monkeypatch.setenv("EKF_SIM_PARALLEL", env)
        e3 = pyekf.EKF(n_landmarks=N, n_filters=F)
        sim3 = _sim_for(e3, case)
        assert _bytes(_runs(sim3, case)) == _bytes(parts)
        sim3.close()
        e3.close()
    for h in (sim, e, e2):
        h.close()


# ---- the Joseph form -----------------------------------------------------------------------------
@pytest.mark.parametrize("parallel", ["1", "0"], ids=["parallel", "sequential"])
def test_empty_messages_in_the_joseph_form_on_the_pipeline(monkeypatch, parallel):
    """As test_sim_joseph_on_the_pipeline, over messages with no marker: both forms write kJoseph
    chunks for the messages that have one, against the oracle's Joseph mode."""
    pyekf.poison_lds()
    monkeypatch.setenv("EKF_RESIDENT", "0")
    monkeypatch.setenv("EKF_SIM_PARALLEL", parallel)
    case = sc.get("empty")
    parts, got = _run_form(case, case.n_slots, pyekf.EKF_PATH_PIPELINE, joseph=True)
    if parallel == "1":
        e2 = _twin(case, case.n_slots, parts, known=True, joseph=True)
        for (x, S, c), (x2, S2, c2) in zip(got, _states(e2)):
            assert x.tobytes() == x2.tobytes() and S.tobytes() == S2.tobytes() and c == c2
        e2.close()
    _against_oracle(case, case.n_slots, parts, got, joseph=True)


# ---- rejections ----------------------------------------------------------------------------------
def _refused_create(e, landmarks, kw):
    with pytest.raises(pyekf.EkfError) as err:
        pyekf.Sim(e, landmarks, **kw)
    assert err.value.rc == pyekf.EKF_E_ARG


def test_rejections_leave_the_filter_and_the_simulator_usable():
    pyekf.poison_lds()
    case = sc.get("size-64")
    sw, kw = case.sw, case.sim_kw
    e = pyekf.EKF(n_landmarks=64, n_filters=2)
    # ekf_sim_create
    _refused_create(e, sc.get("size-65").sw.landmarks, kw)                       # n_map > N
    for tpm in (0, 65):
        _refused_create(e, sw.landmarks, {**kw, "ticks_per_msg": tpm})
    _refused_create(e, sw.landmarks, {**kw, "max_markers": 17, "marker_stride": 17})   # L ≥ 17
    _refused_create(e, sw.landmarks, {**kw, "marker_stride": 15})                # stride < m
    big = pyekf.EKF(n_landmarks=1025, n_filters=1)
    _refused_create(big, synth.random_landmarks(1025, 1)[None], kw)
    big.close()
    sim = _sim_for(e, case)
    _runs(sim, case)                                 # the filter still takes a valid simulator
    assert [e.status(f) for f in range(2)] == [0, 0]
    sim.close()
    e.close()

    # ekf_sim_run: refused, the simulator has not moved, and the same run with valid senses follows
    lib = pyekf.lib()
    seventeen = sc._make("seventeen", 17, 64, 2, 3, map_seed=3017, seed=950)
    narrow = sc._make("narrow", 12, 64, 2, 3, map_seed=4200, seed=960, m=3)
    assert sc.guard(seventeen) > sc.GAP and sc.guard(narrow) > sc.GAP and narrow.stride == 3
    for c, bad in ((seventeen, [0, 2, 0]),         # an ALL message with L = 17
                   (narrow, [0, 0, 2]),            # an ALL message with marker_stride < L
                   (seventeen, [0, 3, 0]), (seventeen, [-1, 0, 0])):
        e = pyekf.EKF(n_landmarks=64, n_filters=2)
        sim = _sim_for(e, c)
        cmd = np.ascontiguousarray(c.sw.cmd)
        sense = np.asarray(bad, np.int32)
        assert lib.ekf_sim_run(sim.h, 3, cmd.ctypes.data, sense.ctypes.data) == pyekf.EKF_E_ARG
        x, S, cnt = e.state(0)
        assert cnt == 0 and not x.any()
        _runs(sim, c)
        assert [e.status(f) for f in range(2)] == [0, 0]
        sim.close()
        e.close()
