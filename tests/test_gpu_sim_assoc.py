"""ekf_sim_run_assoc (include/ekf_sim.h): a Monte-Carlo run with unknown association whose inputs
never leave the GPU — the simulator's parallel form into its marker buffers, then
ekf_replay_device_assoc (pipeline handles) or ekf_replay_resident with assoc = 1 (resident handles)
over them, the ids ignored — and ekf_sim_eval_match on what it leaves.

Twins: the same handle fed the run's recorded markers (ekf_sim_markers, ekf_sim_poses) through the
replay underneath must end bit-identical: the run adds no arithmetic of its own. The oracle:
OracleEKF.sensor_cb message by message, under the decision margins of
tests/test_gpu_assoc_device.py (1e-6 relative from the gate and from the runner-up), which are
asserted on the CPU first, on synth.swarm's host restatement of the simulator (device and host
markers agree to about 1e-14 m); poses within that file's 1e-8."""
import numpy as np
import pytest

import pyekf
from pyekf import synth

import test_gpu_assoc_device as tad
import test_gpu_eval as tge
from match_ref import match_np, seen_slots, to_map_frame
from test_gpu_eval_match import MARGIN, permuted, same_record
from test_gpu_sim import _sim_for

pytestmark = pytest.mark.gpu

T = 12
M = 16
POSE_TOL = 1e-8      # tests/test_gpu_assoc_device.py:263


def _handle(N, F, dtype=pyekf.EKF_F64, joseph=False, trace=32):
    e = pyekf.EKF(n_landmarks=N, n_filters=F, dtype=dtype)
    if joseph:
        assert e.set_joseph(True) == 0
    if trace:
        e.trace_enable(trace)
    return e


def _twin_replay(e2, cnt, rel, odom):
    """The recorded run through the replay underneath: counts, packed (x, y) pairs and the
    odometry (every filter's is the commanded one) back on the GPU, ids none."""
    F = cnt.shape[1]
    dev = tge._gpu((cnt, rel, np.repeat(odom[:, None], F, 1)))
    e2.replay_on_device(dev[0], dev[1], dev[2], ids=None)
    e2.sync()            # (the tensors may go once the replay has read them)


def _same(a, b, m=M):
    ra, sa = tge._everything(a, m)
    rb, sb = tge._everything(b, m)
    assert ra == rb
    assert sa == sb


CASES = {  # N, F, dtype, joseph, path
    "pipeline96": (96, 2, pyekf.EKF_F64, False, pyekf.EKF_PATH_PIPELINE),
    "resident50": (50, 3, pyekf.EKF_F64, False, pyekf.EKF_PATH_RESIDENT),
    "pipeline96-joseph": (96, 2, pyekf.EKF_F64, True, pyekf.EKF_PATH_PIPELINE),
    "resident50-joseph": (50, 2, pyekf.EKF_F64, True, pyekf.EKF_PATH_RESIDENT),
    "f32-96": (96, 2, pyekf.EKF_F32, False, pyekf.EKF_PATH_PIPELINE),
}


def _run_and_twin(name, n_msgs=T):
    N, F, dtype, joseph, path = CASES[name]
    sw = synth.swarm(N, F, T + 4, survey=False)
    tpm = sw.wheel.shape[1]
    e = _handle(N, F, dtype, joseph)
    assert e.path == path
    sim = _sim_for(e, sw)
    sim.run_assoc(sw.cmd[:n_msgs * tpm])
    cnt, ids, act, rel = sim.markers()
    odom, truth = sim.poses()
    assert cnt.shape == (n_msgs, F) and (cnt > 0).all()
    e2 = _handle(N, F, dtype, joseph)
    _twin_replay(e2, cnt, rel, odom)
    _same(e, e2)
    assert all(e.trace_count(f) == n_msgs for f in range(F))
    e2.close()
    return sw, e, sim, (cnt, ids, act, rel, odom, truth)


# ---- 5: twins, and 8: the run scored end to end --------------------------------------------------

@pytest.mark.parametrize("name", ["pipeline96", "resident50"])
def test_run_assoc_equals_the_replay_of_its_own_markers(name):
    pyekf.poison_lds()
    N, F, dtype, _, _ = CASES[name]
    sw, e, sim, (cnt, ids, act, rel, odom, truth) = _run_and_twin(name)
    tpm = sw.wheel.shape[1]
    # the markers are those of a known-id run with the same seed, bit for bit
    e3 = _handle(N, F, dtype, trace=0)
    sim3 = _sim_for(e3, sw)
    sim3.run(sw.cmd[:T * tpm])
    for a, b in zip(sim3.markers() + sim3.poses(), (cnt, ids, act, rel, odom, truth)):
        assert a.tobytes() == b.tobytes()
    assert (ids[:, :, 0] >= 0).all() and (act == 0).all()
    sim3.close()
    e3.close()

    # 8: the run scored against the simulator's truth, slots matched on the device
    start = np.array(sw.start_pose, np.float64)
    max_dist = 0.3
    recs, mrecs, match = sim.eval_match(max_dist)
    assert (mrecs["n_matched"] > 0).all()
    assert (mrecs["n_dup"] == mrecs["n_matched"] - mrecs["n_primary"]).all()
    assert (mrecs["n_missed"] == mrecs["n_truth"] - mrecs["n_primary"]).all()
    assert (mrecs["n_spurious"] == recs["n_seen"] - mrecs["n_matched"]).all()
    assert (mrecs["n_truth"] == N).all() and (recs["n_eval"] == mrecs["n_matched"]).all()
    print(name, "match records:", mrecs)
    for f in range(F):
        x, _, _ = e.state(f, sigma=False)
        xy = x[3:].reshape(N, 2)
        want_match, want, best, second = match_np(xy, to_map_frame(sw.landmarks[f], start),
                                                  max_dist)
        s = seen_slots(xy)
        gate2 = max_dist * max_dist
        close = s & ~((second - best > MARGIN * second) & (np.abs(best - gate2) > MARGIN * gate2))
        assert not close.any(), (f, np.flatnonzero(close))   # the margins, on the CPU
        assert (match[f] == want_match).all(), f
        same_record(mrecs[f], want, True, (name, f))
    # the record: ekf_eval fed the last true pose and the map in slot order
    want = e.eval(truth[-1], permuted(sw.landmarks, match), frame=start)
    assert recs.tobytes() == want.tobytes()

    # split: 7 + 5 messages end as the single call did, and a third call (buffer 0 again) on both
    es = _handle(N, F, dtype)
    sims = _sim_for(es, sw)
    sims.run_assoc(sw.cmd[:7 * tpm])
    sims.run_assoc(sw.cmd[7 * tpm:T * tpm])
    _same(e, es)
    sims.run_assoc(sw.cmd[T * tpm:(T + 4) * tpm])
    sim.run_assoc(sw.cmd[T * tpm:(T + 4) * tpm])
    for a, b in zip(sims.markers() + sims.poses(), sim.markers() + sim.poses()):
        assert a.tobytes() == b.tobytes()
    _same(e, es)
    assert all(e.trace_count(f) == T + 4 for f in range(F))
    for s_, e_ in ((sims, es), (sim, e)):
        s_.close()
        e_.close()


def test_run_assoc_alternates_with_run():
    """ekf_sim_run and ekf_sim_run_assoc on one simulator advance the same counters: the markers of
    run, run_assoc, run are those of one known-id run over the whole drive."""
    pyekf.poison_lds()
    N, F = 96, 2
    sw = synth.swarm(N, F, T, survey=False)
    tpm = sw.wheel.shape[1]
    e, e0 = _handle(N, F), _handle(N, F, trace=0)
    sim, sim0 = _sim_for(e, sw), _sim_for(e0, sw)
    sim0.run(sw.cmd)
    whole = sim0.markers() + sim0.poses()
    parts = []
    for k, (a, b) in enumerate(((0, 4), (4, 9), (9, T))):
        (sim.run_assoc if k == 1 else sim.run)(sw.cmd[a * tpm:b * tpm])
        parts.append(sim.markers() + sim.poses())
    for w, p in zip(whole, (np.concatenate(p) for p in zip(*parts))):
        assert w.tobytes() == p.tobytes()
    assert all(e.trace_count(f) == T for f in range(F))
    for s_, e_ in ((sim, e), (sim0, e0)):
        s_.close()
        e_.close()


# ---- 6: the oracle -------------------------------------------------------------------------------

def test_run_assoc_message_by_message_against_the_oracle():
    pyekf.poison_lds()
    N = tad.N
    sw = synth.swarm(N, 1, T, survey=False)
    # on the CPU: every decision of this seed clears the margins (asserted inside _oracle_drive)
    od = pyekf.odometry(sw.scenario(0))
    _, dec, poses = tad._oracle_drive(sw.count[:, 0], sw.rel[:, 0], od)
    assert sum(int(nw.sum()) for _, nw in dec) > 10 and any((nw == 0).any() for _, nw in dec)
    e = _handle(N, 1, trace=0)
    assert e.path == pyekf.EKF_PATH_PIPELINE
    sim = _sim_for(e, sw)
    tpm = sw.wheel.shape[1]
    worst = 0.0
    for t in range(T):
        sim.run_assoc(sw.cmd[t * tpm:(t + 1) * tpm])
        c = int(sw.count[t, 0])
        j, nw = e.decisions(c)
        assert (j == dec[t][0]).all() and (nw == dec[t][1]).all(), t
        worst = max(worst, float(np.abs(e.pose() - poses[t]).max()))
        assert np.abs(sim.markers()[3][0, 0] - sw.rel[t, 0]).max() < 1e-12
    print(f"worst pose difference to the oracle over {T} messages: {worst:.3g}")
    assert worst < POSE_TOL
    assert e.status() == 0
    sim.close()
    e.close()


# ---- 7: forms and rejections ---------------------------------------------------------------------

@pytest.mark.parametrize("name", ["pipeline96-joseph", "resident50-joseph", "f32-96"])
def test_other_forms_equal_their_replay_twin(name):
    pyekf.poison_lds()
    _, e, sim, _ = _run_and_twin(name, n_msgs=5)
    sim.close()
    e.close()


def _rejected(e, sw, **kw):
    """ekf_sim_run_assoc refused: EKF_E_ARG, and the handle and the simulator as they were."""
    tpm = sw.wheel.shape[1]
    sim = _sim_for(e, sw, **kw)
    before = tge._everything(e, M)
    cmd = np.ascontiguousarray(sw.cmd[:2 * tpm])
    assert pyekf.lib().ekf_sim_run_assoc(sim.h, 2, cmd.ctypes.data) == pyekf.EKF_E_ARG
    assert tge._everything(e, M) == (before[0], [0] * e.F)
    # the simulator has not moved: a known-id run still starts at message 0
    sim.run(sw.cmd[:2 * tpm])
    assert (sim.markers()[0] == sw.count[:2]).all()
    assert np.abs(sim.markers()[3][..., :sw.rel.shape[2], :] - sw.rel[:2]).max() < 1e-9
    sim.close()


def test_rejections(monkeypatch):
    pyekf.poison_lds()
    N, F = 96, 2
    sw = synth.swarm(N, F, 4, survey=False)
    tpm = sw.wheel.shape[1]
    L = pyekf.lib()
    e = _handle(N, F)
    sim = _sim_for(e, sw)
    cmd = np.ascontiguousarray(sw.cmd)
    assert L.ekf_sim_run_assoc(sim.h, -1, cmd.ctypes.data) == pyekf.EKF_E_ARG
    assert L.ekf_sim_run_assoc(sim.h, 2, None) == pyekf.EKF_E_ARG
    assert L.ekf_sim_run_assoc(sim.h, 0, None) == pyekf.EKF_OK
    assert all(e.trace_count(f) == 0 for f in range(F))
    sim.close()
    # a marker stride beyond the replays' 64
    sim = pyekf.Sim(e, sw.landmarks, seed=int(sw.seeds[0]), ticks_per_msg=tpm, max_markers=16,
                    marker_stride=65, start_theta=sw.start_pose[0], start_x=sw.start_pose[1],
                    start_y=sw.start_pose[2], record=1)
    before = tge._everything(e, M)
    assert L.ekf_sim_run_assoc(sim.h, 2, cmd.ctypes.data) == pyekf.EKF_E_ARG
    assert tge._everything(e, M) == (before[0], [0] * F)
    sim.close()
    e.close()
    # strides up to 64 run, on both paths (the marker buffers are allocated for them)
    for n, path in ((96, pyekf.EKF_PATH_PIPELINE), (50, pyekf.EKF_PATH_RESIDENT)):
        sw2 = synth.swarm(n, F, 4, survey=False)
        e = _handle(n, F)
        assert e.path == path
        sim = pyekf.Sim(e, sw2.landmarks, seed=int(sw2.seeds[0]), ticks_per_msg=tpm,
                        max_markers=16, marker_stride=64, start_theta=sw2.start_pose[0],
                        start_x=sw2.start_pose[1], start_y=sw2.start_pose[2], record=1)
        sim.run_assoc(sw2.cmd)
        cnt, _, _, rel = sim.markers()
        e2 = _handle(n, F)
        _twin_replay(e2, cnt, rel, sim.poses()[0])
        _same(e, e2)
        for h in (sim, e, e2):
            h.close()
    # a pipeline handle forced to the one-marker route has no device-planned association replay
    monkeypatch.setenv("EKF_ASSOC_MSG", "0")
    e = _handle(N, F)
    assert e.path == pyekf.EKF_PATH_PIPELINE and e.assoc_route == pyekf.EKF_ASSOC_MARKER
    _rejected(e, sw)
    e.close()
