"""The staged rebuild operands (StageRec → the chain's LDS blocks) at the places they can go wrong.

A kLook chain rebuilds its |U| × |U| block from three blocks over U (its own index set) and U' (the
previous chunk's): D = Σ[U, U], R = Σ[U, U'] and C = Σ[U', U] (kept transposed in LDS), zero-padded
to 36 columns for the MFMA k loop. k_stage writes them two chunks ahead in the layout of the
chain's LDS arrays (RebuildImage) and the chain copies them in; the first two chunks of a call and
EKF_STAGE=0 chains gather the same values themselves. What the hand-over can get wrong: |U| ≠ |U'|
(the zero columns k ≥ |U'|), the padding, the transposed C, a previous chunk without a predict (the second
chunk of a long message) and a chunk whose stage was skipped (a hole in the messages).

One filter, N = 64 landmarks (n = 131, on the HBM pipeline), 14 known-id messages from the state
of an fp64 survey that sighted every landmark, with 16 → 1 → 16 → 2 markers, an empty message,
15, 20 (two chunks) and one message that names a landmark twice; consecutive messages share some
landmarks and not others. Every run starts behind poisoned LDS. Staged and EKF_STAGE=0 runs must
agree bit for bit, and both with the oracle within the bounds of tests/test_gpu_parity.py (fp64)
and tests/test_gpu_scale.py (fp32) — imported, not restated. The oracle-only test pins the
script's properties on the CPU, so a GPU failure is the kernels'.
"""
import numpy as np
import pytest

import orc
import pyekf
from edge_scenarios import oracle_odometry
from pyekf import synth
from test_gpu_parity import POSE_TOL, SIGMA_TOL
from test_gpu_scale import F32_POSE_TOL, F32_SIGMA_TOL, F32_STATE_TOL

N = 64
PATTERN = (16, 1, 16, 2, 0, 16, 15, 20, 16, 16, 3, 16, 16, 16)  # markers per message
HOLE_T, LONG_T, DUP_T = 4, 7, 9
_CACHE = {}


def _script():
    """(count, ids, actions, rel, odom, start state) of the 14 messages, built once."""
    if "script" in _CACHE:
        return _CACHE["script"]
    T = len(PATTERN)
    sc = synth.populated(N, T, max_markers=20)
    odom = oracle_odometry(sc)
    w, M = sc.n_warm, sc.ids.shape[1]
    ref = orc.OracleEKF(n_landmarks=N)
    for t in range(w):
        ref.set_odom(odom[t])
        c = int(sc.count[t])
        ref.fake_sensor_cb(sc.ids[t, :c], sc.actions[t, :c], sc.rel[t, :c])
    x, S, tmo, cnt = ref.get()
    count = np.zeros(T, np.int32)
    ids = np.full((T, M), -1, np.int32)
    act = np.zeros((T, M), np.int32)
    rel = np.zeros((T, M, 2))
    for t, c in enumerate(PATTERN):
        have = int(sc.count[w + t])
        o = 0 if c == 20 else 2 * (t % 3)  # a sliding window of the message's markers
        assert o + c <= have
        count[t] = c
        ids[t, :c] = sc.ids[w + t, o:o + c]
        act[t, :c] = sc.actions[w + t, o:o + c]
        rel[t, :c] = sc.rel[w + t, o:o + c]
    # the same landmark twice in one message: its index pair repeats in U
    ids[DUP_T, 5] = ids[DUP_T, 2]
    rel[DUP_T, 5] = rel[DUP_T, 2] + 1e-3
    _CACHE["script"] = (count, ids, act, rel, np.ascontiguousarray(odom[w:w + T]),
                        (x, S, tmo, cnt))
    return _CACHE["script"]


def _oracle(joseph):
    key = ("oracle", joseph)
    if key not in _CACHE:
        count, ids, act, rel, odom, (x, S, tmo, cnt) = _script()
        ref = orc.OracleEKF(n_landmarks=N, joseph=joseph)
        ref.set(x, S, tmo, x[:3], cnt)
        rcs = []
        for t in range(len(count)):
            ref.set_odom(odom[t])
            c = int(count[t])
            rcs.append(ref.fake_sensor_cb(ids[t, :c], act[t, :c], rel[t, :c]))
        xr, Sr, _, _ = ref.get()
        xr.setflags(write=False)
        Sr.setflags(write=False)
        _CACHE[key] = (xr, Sr, rcs)
    return _CACHE[key]


@pytest.mark.parametrize("joseph", [False, True], ids=["simple", "joseph"])
def test_script_reaches_the_cases_on_the_oracle(joseph):
    """The script alone, on the CPU: every landmark it names is initialised before it starts (no
    first sighting against the 1e7 prior inside it), the oracle accepts every message but the
    empty one and ends finite; the marker counts differ both ways between neighbours, one message
    is empty, one has two chunks, one repeats a landmark, and neighbours share some ids only."""
    count, ids, act, rel, odom, (x, S, tmo, cnt) = _script()
    assert np.all(np.isfinite(x)) and np.all(np.isfinite(S))
    named = np.unique(ids[ids >= 0])
    assert named.min() >= 0 and named.max() < N
    lm = x[3:].reshape(-1, 2)
    assert np.all(np.any(lm[named] != 0.0, 1))
    assert tuple(count) == PATTERN and count[HOLE_T] == 0
    assert count[LONG_T] > 16  # two chunks, the second without a predict
    assert np.all(act[ids >= 0] == synth.ADD)
    d = ids[DUP_T, :count[DUP_T]]
    assert len(np.unique(d)) == len(d) - 1
    for t in range(1, len(count)):
        a, b = set(ids[t - 1, :count[t - 1]]), set(ids[t, :count[t]])
        if len(a) >= 15 and len(b) >= 15:
            assert a & b and a ^ b, t
    xr, Sr, rcs = _oracle(joseph)
    assert [rc == 0 for rc in rcs] == [t != HOLE_T for t in range(len(count))]
    assert np.all(np.isfinite(xr)) and np.all(np.isfinite(Sr))


def _gpu(dtype, joseph, devsync, stage, monkeypatch):
    count, ids, act, rel, odom, (x, S, tmo, cnt) = _script()
    for k in ("EKF_SERIAL", "EKF_CU_SPLIT", "EKF_DEVSYNC", "EKF_STAGE", "EKF_RESIDENT"):
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("EKF_RESIDENT", "0")
    monkeypatch.setenv("EKF_DEVSYNC", devsync)
    monkeypatch.setenv("EKF_STAGE", stage)
    pyekf.poison_lds()  # inherited LDS cannot stand in for padding the image failed to supply
    e = pyekf.EKF(n_landmarks=N, dtype=dtype)
    assert e.path == pyekf.EKF_PATH_PIPELINE
    e.set_state(x, S, tmo=tmo, counter=cnt)
    assert e.set_joseph(joseph) == pyekf.EKF_OK
    e.replay(count[:, None], rel[:, None], odom[:, None], ids=ids[:, None], actions=act[:, None])
    xg, Sg, _ = e.state()
    status = e.status()
    e.close()
    return xg, Sg, status


@pytest.mark.gpu
@pytest.mark.parametrize("devsync", ["1", "0"], ids=["devsync", "events"])
@pytest.mark.parametrize("joseph", [False, True], ids=["simple", "joseph"])
@pytest.mark.parametrize("dtype", [pyekf.EKF_F64, pyekf.EKF_F32], ids=["f64", "f32"])
def test_staged_image_equals_gather_and_oracle(dtype, joseph, devsync, monkeypatch):
    xs, Ss, sts = _gpu(dtype, joseph, devsync, "1", monkeypatch)
    xg, Sg, stg = _gpu(dtype, joseph, devsync, "0", monkeypatch)
    xr, Sr, _ = _oracle(joseph)
    f64 = dtype == pyekf.EKF_F64
    for name, x, S in (("staged", xs, Ss), ("gather", xg, Sg)):
        print(f"{name} {'f64' if f64 else 'f32'} joseph={joseph} devsync={devsync}: "
              f"pose {np.abs(x[:3] - xr[:3]).max():.3e} state {np.abs(x - xr).max():.3e} "
              f"sigma {np.abs(S - Sr).max():.3e}")
    assert sts == 0 and stg == 0
    np.testing.assert_array_equal(xs, xg)
    np.testing.assert_array_equal(Ss, Sg)
    for x, S in ((xs, Ss), (xg, Sg)):
        assert np.all(np.isfinite(x)) and np.all(np.isfinite(S))
        if f64:
            assert np.abs(x - xr).max() < POSE_TOL
            assert np.abs(S - Sr).max() < SIGMA_TOL
        else:
            assert np.abs(x[:3] - xr[:3]).max() < F32_POSE_TOL
            assert np.abs(x - xr).max() < F32_STATE_TOL
            assert np.abs(S - Sr).max() < F32_SIGMA_TOL
