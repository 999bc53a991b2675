"""k_chain's two wave-0 programs on the GPU: same bits, and each where it belongs.

The chain kernel's sequential wave runs a chunk's corrections in a lean program (the common case
alone) and hands the chunk to the generic program at the first marker that is anything else; the
generic program resumes in mid-chunk from what the block in LDS holds. Every drive of
tests/chain_cases.py (pinned by tests/test_chain_cases.py) and the rare-path drives of
tests/edge_scenarios.py run twice on the HBM pipeline (EKF_RESIDENT=0), with EKF_CHAIN_FAST=1 (the
lean program, off by default) and with EKF_CHAIN_FAST=0 (the generic program from step 0, as
before there were two):

* state, Σ, t_map_odom and every posterior pose are byte-equal between the two runs;
* the result agrees with the oracle within edge_scenarios' bounds (KNOWN_TOL fp64, F32_TOL fp32);
* ekf_chain_path_counts, read after every message: lean + generic = the message's corrections;
  the lean program ran each chunk's markers before its first rare event and the generic one the
  rest — so generic = 0 on the clean drives and on every chunk without an event, and ≥ 1 exactly
  in the chunks the CPU test located — and under EKF_CHAIN_FAST=0 lean = 0.

fp64 and fp32, simple and Joseph form, the default schedule and one stream (EKF_SERIAL=1).
"""
import numpy as np
import pytest

import chain_cases as cc
import edge_scenarios as es
import pyekf

pytestmark = pytest.mark.gpu

ENV_KEYS = ("EKF_RESIDENT", "EKF_SERIAL", "EKF_CU_SPLIT", "EKF_DEVSYNC", "EKF_STAGE",
            "EKF_ASSOC_MSG", "EKF_AM_XCD", "EKF_CHAIN_FAST")
SCHEDULES = {"default": {}, "serial": {"EKF_SERIAL": "1"}}
FORMS = pytest.mark.parametrize("joseph", [False, True], ids=["simple", "joseph"])
DTYPES = pytest.mark.parametrize("dtype", [pyekf.EKF_F64, pyekf.EKF_F32], ids=["f64", "f32"])
SCHEDS = pytest.mark.parametrize("sched", list(SCHEDULES))
NUMERIC, RANGE = pyekf.EKF_FLAG_NUMERIC, pyekf.EKF_FLAG_RANGE
_oracle: dict = {}


def _ref(name, joseph):
    if (name, joseph) not in _oracle:
        _oracle[name, joseph] = cc.locate(cc.get(name), joseph)
    return _oracle[name, joseph]


def _env(monkeypatch, sched, fast):
    for k in ENV_KEYS:
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("EKF_RESIDENT", "0")
    for k, v in SCHEDULES[sched].items():
        monkeypatch.setenv(k, v)
    monkeypatch.setenv("EKF_CHAIN_FAST", "1" if fast else "0")


def _handle(n_landmarks, dtype, joseph, start):
    h = pyekf.EKF(n_landmarks=n_landmarks, dtype=dtype)
    assert h.path == pyekf.EKF_PATH_PIPELINE
    assert h.set_joseph(joseph) == pyekf.EKF_OK
    assert h.chain_path_counts() == (0, 0)
    if start is not None:
        x, S, tmo, cnt = start
        h.set_state(x, S, tmo=tmo, counter=cnt)
    return h


def _run(case, dtype, joseph):
    """The case through a fresh handle → dict(x, S, tmo, counter, poses [T, 3], counts [T, 2]: the
    step counters' increments per message (a device replay: its total in row T − 1), status [T])."""
    e = case.edge
    T = e.n_messages
    h = _handle(e.n_landmarks, dtype, joseph, case.start)
    poses, counts, status = np.zeros((T, 3)), np.zeros((T, 2), np.int64), np.zeros(T, np.int64)
    if case.how == "sensor":
        last = np.zeros(2, np.int64)
        for t in range(T):
            c = int(e.count[t])
            assert h.set_odom(e.odom[t]) == 0
            assert h.fake_sensor(e.ids[t, :c], e.actions[t, :c], e.rel[t, :c]) == 0
            now = np.array(h.chain_path_counts(), np.int64)
            counts[t], last = now - last, now
            status[t] = h.status()
            poses[t] = h.pose()
    else:
        import torch
        M = e.ids.shape[1]
        arrs = (e.count[:, None], e.rel[:, None], e.odom[:, None], e.ids[:, None],
                e.actions[:, None])
        g = [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in arrs]
        assert M <= cc.CHUNK
        h.replay_device(*g)
        counts[T - 1] = h.chain_path_counts()   # (synchronises: the tensors may go)
        status[T - 1] = h.status()
        poses[T - 1] = h.pose()
    x, S, cnt = h.state()
    out = dict(x=x, S=S, tmo=h.map_odom(), counter=cnt, poses=poses, counts=counts, status=status)
    h.reset()
    assert h.chain_path_counts() == (0, 0)   # ekf_reset clears the counters
    h.close()
    return out


def _same_bits(a, b):
    for k in ("x", "S", "tmo", "poses"):
        np.testing.assert_array_equal(a[k], b[k], err_msg=k)
    assert a["counter"] == b["counter"]
    np.testing.assert_array_equal(a["status"], b["status"])


def _against_oracle(got, ref, dtype, last_pose_only=False):
    pt, st, sg = es.F32_TOL if dtype == pyekf.EKF_F32 else es.KNOWN_TOL
    assert np.all(np.isfinite(got["x"])) and np.all(np.isfinite(got["S"]))
    assert got["counter"] == ref["counter"]
    rows = slice(-1, None) if last_pose_only else slice(None)
    err = dict(pose=float(np.abs(got["poses"][rows] - ref["poses"][rows]).max()),
               state=float(np.abs(got["x"] - ref["state"]).max()),
               tmo=float(np.abs(got["tmo"] - ref["tmo"]).max()),
               sigma=float(np.abs(got["S"] - ref["sigma"]).max()))
    print(err)
    assert err["pose"] < pt and err["tmo"] < st and err["state"] < st and err["sigma"] < sg, err


@SCHEDS
@FORMS
@DTYPES
@pytest.mark.parametrize("name", [n for n in cc.CASES if cc.get(n).how == "sensor"] + cc.EDGE_CASES)
def test_per_message(monkeypatch, name, dtype, joseph, sched):
    case, ref = cc.get(name), _ref(name, joseph)
    e = case.edge
    _env(monkeypatch, sched, fast=True)
    pyekf.poison_lds()
    a = _run(case, dtype, joseph)
    _env(monkeypatch, sched, fast=False)
    b = _run(case, dtype, joseph)
    _same_bits(a, b)
    _against_oracle(a, ref, dtype)
    np.testing.assert_array_equal(a["status"], np.where(ref["rcs"] == es.NUMERIC, NUMERIC, 0))
    want = cc.expected_counts(case, ref["events"])
    print(a["counts"].tolist(), want.tolist())
    np.testing.assert_array_equal(a["counts"].sum(1), e.count)
    np.testing.assert_array_equal(a["counts"], want)
    np.testing.assert_array_equal(b["counts"][:, 0], 0)
    np.testing.assert_array_equal(b["counts"][:, 1], e.count)
    if name in cc.CLEAN:
        assert a["counts"][:, 1].sum() == 0
    else:  # the generic program ran in exactly the messages with an event
        hit = sorted({t for t, _ in ref["events"]})
        assert sorted(np.flatnonzero(a["counts"][:, 1]).tolist()) == hit


@SCHEDS
@FORMS
@DTYPES
def test_id_out_of_range_in_mid_chunk(monkeypatch, dtype, joseph, sched):
    """ekf_replay_device hands the kernel an id beyond the map at position 5 of a 16-marker chunk
    (the host forms refuse it; the oracle's fake_sensor_cb refuses the whole message): the marker
    is skipped with EKF_FLAG_RANGE, by the generic program from that step on; compared with the
    forced-generic run."""
    case, ref = cc.get("badid_p5"), _ref("badid_p5", joseph)
    e = case.edge
    _env(monkeypatch, sched, fast=True)
    a = _run(case, dtype, joseph)
    _env(monkeypatch, sched, fast=False)
    b = _run(case, dtype, joseph)
    _same_bits(a, b)
    assert a["status"][-1] == RANGE
    want = cc.expected_counts(case, ref["events"]).sum(0)
    assert a["counts"][-1].tolist() == want.tolist() == [int(e.count.sum()) - 11, 11]
    assert b["counts"][-1].tolist() == [0, int(e.count.sum())]
    # (the skipped marker changes nothing, as the oracle's per-marker -2: its run is a reference
    # all the same)
    _against_oracle(a, ref, dtype, last_pose_only=True)


@SCHEDS
@FORMS
@DTYPES
@pytest.mark.parametrize("turns", [5, -5])
def test_heading_state(monkeypatch, turns, dtype, joseph, sched):
    """ekf_set_state with a heading of about +-31 rad, ekf_correct per marker (one chunk each, no
    predict): the first correction's bearing and heading are beyond normalize_angle_near's range —
    the lean program leaves at step 0 and the generic one's fallbacks run — every later one is the
    lean program's."""
    hs = es.heading_state(turns)
    x0, S0, tmo0, od, ids, rel = hs
    xr, Sr, tmr, pr = es.run_heading_state(hs, joseph=joseph)
    kinds, _ = cc.locate_heading_state(hs, joseph)
    want = np.array([[0, 1] if k else [1, 0] for k in kinds], np.int64)
    out = []
    for fast in (True, False):
        _env(monkeypatch, sched, fast)
        h = _handle((x0.shape[0] - 3) // 2, dtype, joseph, (x0, S0, tmo0, 0))
        assert h.set_odom(od) == 0
        poses, counts, last = [], [], np.zeros(2, np.int64)
        for lid, (rx, ry) in zip(ids, rel):
            assert h.correct(lid, rx, ry) == 0
            now = np.array(h.chain_path_counts(), np.int64)
            counts.append(now - last)
            last = now
            poses.append(h.pose())
        assert h.posterior() == 0
        x, S, cnt = h.state()
        out.append(dict(x=x, S=S, tmo=h.map_odom(), counter=cnt, poses=np.array(poses),
                        counts=np.array(counts), status=np.array([h.status()])))
        h.close()
    a, b = out
    _same_bits(a, b)
    assert a["status"][0] == 0
    _against_oracle(a, dict(poses=pr, state=xr, sigma=Sr, tmo=tmr, counter=0), dtype)
    np.testing.assert_array_equal(a["counts"], want)
    assert want[:, 1].tolist() == [1] + [0] * (len(ids) - 1)
    np.testing.assert_array_equal(b["counts"], np.array([[0, 1]] * len(ids)))
