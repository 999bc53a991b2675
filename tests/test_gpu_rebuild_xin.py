"""k_chain's rebuild on the GPU: x_in[U] and the bands of K', M' and P.

A chunk after the first of a pipelined replay rebuilds its block Σ_in[U, U] and its state x_in[U]
from the chunk before (kLook): x_in[u_a] is the previous chunk's x[U'] at the position of u_a in
U' — a map the chain builds with its index sets — or, for a column the previous chunk did not
touch, x'[u_a] + R[a]·Zx'. The drives below pin down how U and U' can relate, at N = 50 with 5–8
messages each (one chunk a message), every message after the first a rebuilding chunk:

  same          U = U' (the same three landmarks every message)
  pose_only     U and U' share only the pose (two disjoint pairs of landmarks in turn)
  one_missing   one landmark of U is not in U' but was sighted before: the x' + R·Zx' branch
  twice         a landmark sighted twice (and three times) in one message, in U and in U'
  m1, m2        one and two markers a message (|U| = 5, 7), changing landmarks
  sizes         |U'| ≠ |U|: 4, 1, 2, 6, 1, 3 markers
  full16        16 markers (|U| = 35: the three band rows / columns beside the MFMA tiles), then 15
                and 16 others, so that U' has positions 32..34 that U lacks and the reverse

Each drive, fp64 and fp32, simple and Joseph form, is checked four ways: bit-identical across the
three schedules (default, EKF_DEVSYNC=0, EKF_SERIAL=1), with the chain gathering its own operands
(EKF_STAGE=0), and with wave 0's lean program (EKF_CHAIN_FAST=1); and against the C oracle at
tests/test_gpu_parity.py's bounds (fp64: its POSE_TOL for the state and SIGMA_TOL for Σ, which
tests/edge_scenarios.py keeps as KNOWN_TOL; fp32 Σ: the fp32 bounds it keeps as F32_TOL).
"""
import numpy as np
import pytest

import edge_scenarios as es
import orc
import pyekf

pytestmark = pytest.mark.gpu

N = 50
ENV_KEYS = ("EKF_RESIDENT", "EKF_SERIAL", "EKF_CU_SPLIT", "EKF_DEVSYNC", "EKF_STAGE",
            "EKF_ASSOC_MSG", "EKF_AM_XCD", "EKF_CHAIN_FAST")

_R16 = list(range(16))
DRIVES = {
    "same": [[0, 1, 2]] * 6,
    "pose_only": [[0, 1], [2, 3], [0, 1], [2, 3], [0, 1], [2, 3]],
    "one_missing": [[0, 1, 2], [0, 1, 3], [0, 1, 2], [0, 1, 3], [4, 1, 0], [0, 2, 4]],
    "twice": [[0, 1, 0], [1, 0, 1, 1], [2, 2], [0, 2, 0, 1], [1, 1, 2], [0, 1, 2]],
    "m1": [[0], [0], [1], [0], [1], [2], [2]],
    "m2": [[0, 1], [1, 2], [2, 0], [0, 1], [3, 1], [1, 3], [0, 2]],
    "sizes": [[0, 1, 2, 3], [0], [1, 2], [0, 1, 2, 3, 4, 5], [5], [3, 4, 0], [0, 1, 2, 3], [2]],
    "full16": [_R16, _R16[1:], [16] + _R16[:15], _R16, list(range(4, 20)), _R16[::-1]],
}


def _messages(name):
    """→ counts [T], ids [T, M], rel [T, M, 2], odom [T, 3]: 20 landmarks on two rings, the robot on
    a gentle arc (the odometry is the truth), markers with 1 mm noise."""
    lists = DRIVES[name]
    T, M = len(lists), max(len(l) for l in lists)
    rng = np.random.default_rng(sorted(DRIVES).index(name))
    ang = 2 * np.pi * np.arange(20) / 20
    ring = 2.0 + (np.arange(20) % 2)
    lm = np.stack([ring * np.cos(ang), ring * np.sin(ang)], 1)
    counts = np.array([len(l) for l in lists], np.int32)
    ids, rel, odom = np.zeros((T, M), np.int32), np.zeros((T, M, 2)), np.zeros((T, 3))
    for t, l in enumerate(lists):
        th, px, py = 0.05 * (t + 1), 0.08 * (t + 1), 0.03 * (t + 1)
        odom[t] = (th, px, py)
        d = lm[l] - (px, py)
        c, s = np.cos(th), np.sin(th)
        rel[t, :len(l)] = np.stack([c * d[:, 0] + s * d[:, 1], -s * d[:, 0] + c * d[:, 1]], 1) \
            + rng.normal(0, 1e-3, (len(l), 2))
        ids[t, :len(l)] = l
    return counts, ids, rel, odom


_runs: dict = {}
_refs: dict = {}


def _run(monkeypatch, name, dtype, joseph, env=()):
    """The drive in one pipelined replay → (x, Σ, t_map_odom); once per setting."""
    key = (name, dtype, joseph, tuple(env))
    if key not in _runs:
        for k in ENV_KEYS:
            monkeypatch.delenv(k, raising=False)
        monkeypatch.setenv("EKF_RESIDENT", "0")
        for k, v in env:
            monkeypatch.setenv(k, v)
        counts, ids, rel, odom = _messages(name)
        if not env:
            pyekf.poison_lds()
        e = pyekf.EKF(n_landmarks=N, dtype=dtype)
        assert e.path == pyekf.EKF_PATH_PIPELINE
        assert e.set_joseph(joseph) == pyekf.EKF_OK
        e.replay(counts[:, None], rel[:, None], odom[:, None], ids=ids[:, None],
                 actions=np.zeros_like(ids)[:, None])
        x, S, _ = e.state()
        assert e.status() == 0, key
        _runs[key] = (x, S, e.map_odom())
        e.close()
    return _runs[key]


def _oracle(name, joseph):
    if (name, joseph) not in _refs:
        counts, ids, rel, odom = _messages(name)
        ref = orc.OracleEKF(n_landmarks=N, joseph=joseph)
        for t in range(len(counts)):
            c = int(counts[t])
            ref.set_odom(odom[t])
            assert ref.fake_sensor_cb(ids[t, :c], np.zeros(c, np.int32), rel[t, :c]) == 0
        _refs[name, joseph] = ref.get()[:2]
    return _refs[name, joseph]


def _same_bits(a, b):
    for u, v, what in zip(a, b, ("x", "S", "tmo")):
        np.testing.assert_array_equal(u, v, err_msg=what)


CASES = [pytest.mark.parametrize("name", list(DRIVES)),
         pytest.mark.parametrize("dtype", [pyekf.EKF_F64, pyekf.EKF_F32], ids=["f64", "f32"]),
         pytest.mark.parametrize("joseph", [False, True], ids=["simple", "joseph"])]


def cases(fn):
    for mark in CASES:
        fn = mark(fn)
    return fn


@cases
def test_schedules_same_bits(monkeypatch, name, dtype, joseph):
    dev = _run(monkeypatch, name, dtype, joseph)
    _same_bits(dev, _run(monkeypatch, name, dtype, joseph, (("EKF_DEVSYNC", "0"),)))
    _same_bits(dev, _run(monkeypatch, name, dtype, joseph, (("EKF_SERIAL", "1"),)))


@cases
def test_gathered_operands_same_bits(monkeypatch, name, dtype, joseph):
    """EKF_STAGE=0: the chain gathers the rebuild's operands itself instead of a staged image."""
    _same_bits(_run(monkeypatch, name, dtype, joseph),
               _run(monkeypatch, name, dtype, joseph, (("EKF_STAGE", "0"),)))


@cases
def test_lean_program_same_bits(monkeypatch, name, dtype, joseph):
    """EKF_CHAIN_FAST=1: wave 0's lean program starts from the rebuilt block and x_in[U]."""
    _same_bits(_run(monkeypatch, name, dtype, joseph),
               _run(monkeypatch, name, dtype, joseph, (("EKF_CHAIN_FAST", "1"),)))


@cases
def test_against_oracle(monkeypatch, name, dtype, joseph):
    x, S, _ = _run(monkeypatch, name, dtype, joseph)
    xr, Sr = _oracle(name, joseph)
    _, st, sg = es.F32_TOL if dtype == pyekf.EKF_F32 else es.KNOWN_TOL
    ex, eS = float(np.abs(x - xr).max()), float(np.abs(S - Sr).max())
    print(f"{name}: max |Δx| {ex:.3e} (bound {st:g}), max |ΔΣ| {eS:.3e} (bound {sg:g})")
    assert np.all(np.isfinite(S))
    assert ex < st and eS < sg
