"""The BASELINE configs at their full sizes on populated maps (an untimed warm-up
that initialises every landmark), through the C-ABI, against the C oracle.

* configs[1]: N=256, fp64, one filter — survey + circle vs the oracle.
* configs[2]: N=1024 — the fp64 survey (1 024 first sightings, the only thing fp32 cannot do
  against the 1e7 prior, slam.cpp:130) vs the oracle; then fp32 Σ from that warm state, vs the fp64
  oracle, in the default and the device-epoch schedule.
* configs[3]: N=256 × 512 filters (one GPU's share of 4 096), each seeded base + f: every filter's
  status, a strided sample vs the oracle.
* Association at scale: unknown ids against ≥ 256 known landmarks on the pipeline
  (slam.cpp:344-440), decisions exactly equal to the oracle's.

Tolerances: fp64 pose traces 1e-8; on populated maps state 5e-8 and Σ 1e-7 absolute (1e-14 of
the 1e7 prior, slam.cpp:130). Every first sighting computes a landmark's variance as
1e7 − (1e7 − δ), so two faithful fp64 evaluation orders differ there by ~1e7·ε per sighting: the
two CPU restatements (oracle/ekf_oracle.c literal dense (I − KH)Σ vs structured rank-2) already
differ by 1.8e-8 in Σ on the N=256 populated drive (152 survey + 25 circle messages, 256 first
sightings), so 1e-7 is 5× that floor. The chunked update also carries a chunk's first-sighting
prior into its later corrections' factor products (K_c = r₀·Z_c, x += r₀·Zx), each rounding at
~1e7·ε: the state lands ≈1e-8 from the oracle after a survey (1.0e-9 between the two CPU
restatements), hence 5e-8. fp32 Σ: poses 1e-6, state 1e-5 and Σ 5e-5 absolute against the fp64
oracle (20–40× the measured errors). Measured errors go to gpurun_out/scale_errors.json.
"""
import json
import os

import numpy as np
import pytest

import orc
import pyekf
from pyekf import synth

pytestmark = pytest.mark.gpu

POSE_TOL = 1e-8
STATE_TOL = 5e-8
SIGMA_TOL = 1e-7
# fp32 Σ (configs[2]) against the fp64 oracle from the same warm state: Σ entries are O(1) or
# below on the populated map, so fp32's 6e-8 relative rounding over 16 rank-2 terms per pass and
# 40 passes lands ≈1e-6 absolute (measured, gpurun_out/scale_errors.json)
F32_POSE_TOL = 1e-6
F32_STATE_TOL = 1e-5
F32_SIGMA_TOL = 5e-5
ERRORS = {}


@pytest.fixture(scope="module", autouse=True)
def _record_errors():
    yield
    _write_errors()


def errors_dir():
    """The directory the suite's measured errors go to (tests/edge_scenarios.py writes there too)."""
    out = os.path.join(os.environ.get("GRAFT_REPO_ROOT", "."), "gpurun_out")
    os.makedirs(out, exist_ok=True)
    return out


def _write_errors():
    out = errors_dir()
    with open(os.path.join(out, "scale_errors.json"), "w") as fh:
        json.dump(ERRORS, fh, indent=1)


def _initialised(x):
    """Landmark slots whose state is no longer (0, 0) (the first-sighting test, slam.cpp:213)."""
    return int(np.count_nonzero(np.any(x[3:].reshape(-1, 2) != 0.0, 1)))


def _oracle_from(ws, N):
    x, S, tmo, cnt = ws
    ref = orc.OracleEKF(n_landmarks=N)
    ref.set(x, S, tmo, x[:3], cnt)
    return ref


def _replay(e, sl, sc, odom, assoc=False, poses=False):
    return e.replay(sc.count[sl, None], sc.rel[sl, None], odom[sl, None],
                    ids=None if assoc else sc.ids[sl, None], actions=sc.actions[sl, None],
                    assoc=assoc, poses=poses)


def test_n256_fp64_populated_against_oracle():
    """configs[1]: survey (125 messages, all 256 landmarks) + 25 circle messages, fp64."""
    sc = synth.populated(256, 25)
    s = pyekf.Slam(n_landmarks=256, source=pyekf.SOURCE_SIM)
    rc, poses, tmo = s.replay(sc)
    x, S, cnt = s.filter_state()
    s.close()
    o = orc.run_scenario(sc, False)
    assert rc == 0
    assert _initialised(x) == 256
    ERRORS["n256_fp64"] = {"pose": float(np.abs(poses - o["poses"]).max()),
                           "sigma": float(np.abs(S - o["sigma"]).max())}
    assert np.abs(poses - o["poses"]).max() < POSE_TOL
    assert np.abs(x - o["state"]).max() < STATE_TOL
    assert np.abs(S - o["sigma"]).max() < SIGMA_TOL


@pytest.mark.parametrize("joseph", [False, True], ids=["simple", "joseph"])
@pytest.mark.parametrize("dtype", [pyekf.EKF_F64, pyekf.EKF_F32], ids=["f64", "f32"])
def test_n256_survey_against_oracle(dtype, joseph):
    """configs[1]'s survey at N = 256 (every landmark's first sighting against the 1e7 prior,
    slam.cpp:213-216, plus the circle messages) in both update forms, one chunk of ≤16 markers per
    Joseph message, against the oracle in the same form. fp64 at the fp64 tolerances above. fp32
    keeps Σ in fp32 and takes each first sighting's block from the chain's fp64 patch (the V·Kᵀ
    terms too in the Joseph form, k_chain's pend block); its pose bound is 5e-6 here, not 1e-6:
    measured (r6) simple 9.4e-7 / 3.2e-6 / 2.8e-5 and Joseph 1.9e-6 / 5.8e-6 / 1.4e-5 (pose /
    state / Σ) — 256 first sightings each round Σ's new rows once, on top of the 40-pass walk the
    1e-6 bound is sized for."""
    sc = synth.populated(256, 25)
    odom = pyekf.odometry(sc)
    e = pyekf.EKF(n_landmarks=256, dtype=dtype)
    assert e.path == pyekf.EKF_PATH_PIPELINE
    assert e.set_joseph(joseph) == pyekf.EKF_OK
    _replay(e, slice(0, sc.n_messages), sc, odom)
    x, S, cnt = e.state()
    assert e.status() == 0
    e.close()
    ref = orc.OracleEKF(n_landmarks=256, joseph=joseph)
    for t in range(sc.n_messages):
        ref.set_odom(odom[t])
        c = int(sc.count[t])
        ref.fake_sensor_cb(sc.ids[t, :c], sc.actions[t, :c], sc.rel[t, :c])
    xr, Sr, _, cr = ref.get()
    assert cnt == cr and _initialised(x) == 256
    key = (f"n256_survey_{'joseph' if joseph else 'simple'}_"
           + ("f64" if dtype == pyekf.EKF_F64 else "f32"))
    ERRORS[key] = {"pose": float(np.abs(x[:3] - xr[:3]).max()),
                   "state": float(np.abs(x - xr).max()), "sigma": float(np.abs(S - Sr).max())}
    pt, st, sg = ((POSE_TOL, STATE_TOL, SIGMA_TOL) if dtype == pyekf.EKF_F64 else
                  (5e-6, F32_STATE_TOL, F32_SIGMA_TOL))
    assert np.abs(x[:3] - xr[:3]).max() < pt
    assert np.abs(x - xr).max() < st
    assert np.abs(S - Sr).max() < sg


@pytest.fixture(scope="module")
def n1024():
    """configs[2]'s map: the fp64 survey on the GPU (every landmark sighted), and its state."""
    sc = synth.populated(1024, 40)
    odom = pyekf.odometry(sc)
    w = sc.n_warm
    e = pyekf.EKF(n_landmarks=1024)
    _replay(e, slice(0, w), sc, odom)
    x, S, cnt = e.state()
    ws = (x, S, e.map_odom(), cnt)
    assert e.status() == 0
    e.close()
    return sc, odom, ws


def test_n1024_survey_schedules_bit_identical(n1024, monkeypatch):
    """The first 160 survey messages (many first sightings against the 1e7 prior, heavy index
    overlap between consecutive messages) in one persistent device-epoch replay, in the
    event-synchronised schedule and on one stream, with the chains' rebuild operands staged behind
    the Σ passes (default) and gathered by the chains themselves (EKF_STAGE=0): bit-identical
    states (a chain that carried its own block from chunk to chunk instead of rebuilding it drifted
    from the HBM Σ here and went non-finite)."""
    sc, odom, _ = n1024
    sl = slice(0, 160)
    out = []
    for env in ({"EKF_DEVSYNC": "1"}, {"EKF_DEVSYNC": "0"}, {"EKF_SERIAL": "1"},
                {"EKF_DEVSYNC": "1", "EKF_STAGE": "0"}):
        for k in ("EKF_SERIAL", "EKF_CU_SPLIT", "EKF_DEVSYNC", "EKF_STAGE"):
            monkeypatch.delenv(k, raising=False)
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        e = pyekf.EKF(n_landmarks=1024)
        _replay(e, sl, sc, odom)
        out.append(e.state())
        assert e.status() == 0, env
        e.close()
    for x, S, c in out[1:]:
        np.testing.assert_array_equal(x, out[0][0])
        np.testing.assert_array_equal(S, out[0][1])


def test_n1024_fp64_survey_against_oracle(n1024):
    """All 1 024 first sightings (the 1e7-prior cancellations) on the pipeline vs the oracle."""
    sc, odom, (x, S, tmo, cnt) = n1024
    w = sc.n_warm
    ref = orc.OracleEKF(n_landmarks=1024)
    for t in range(w):
        ref.set_odom(odom[t])
        c = int(sc.count[t])
        ref.fake_sensor_cb(sc.ids[t, :c], sc.actions[t, :c], sc.rel[t, :c])
    xr, Sr, tmr, _ = ref.get()
    assert _initialised(x) == 1024
    ERRORS["n1024_fp64_survey"] = {"state": float(np.abs(x - xr).max()),
                                   "sigma": float(np.abs(S - Sr).max())}
    assert np.abs(x - xr).max() < STATE_TOL
    assert np.abs(tmo - tmr).max() < STATE_TOL
    assert np.abs(S - Sr).max() < SIGMA_TOL


@pytest.mark.parametrize("env", [{"EKF_DEVSYNC": "0"}, {"EKF_DEVSYNC": "1"}],
                         ids=["events", "devsync"])
def test_n1024_fp32_populated_against_oracle(n1024, env, monkeypatch):
    """configs[2]: fp32 Σ over 40 circle messages (640 corrections of a fully correlated 1 024-
    landmark map) from the fp64 survey's state, vs the fp64 oracle from the same state."""
    for k in ("EKF_SERIAL", "EKF_CU_SPLIT", "EKF_DEVSYNC"):
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    sc, odom, ws = n1024
    w, T = sc.n_warm, sc.n_messages - sc.n_warm
    assert _initialised(ws[0]) == 1024
    pyekf.poison_lds()
    e = pyekf.EKF(n_landmarks=1024, dtype=pyekf.EKF_F32)
    x, S, tmo, cnt = ws
    e.set_state(x, S, tmo=tmo, counter=cnt)
    poses = _replay(e, slice(w, w + T), sc, odom, poses=True)
    ref = _oracle_from(ws, 1024)
    err = 0.0
    for t in range(T):
        ref.set_odom(odom[w + t])
        c = int(sc.count[w + t])
        ref.fake_sensor_cb(sc.ids[w + t, :c], sc.actions[w + t, :c], sc.rel[w + t, :c])
        xr = ref.get(sigma=False)[0]
        err = max(err, float(np.abs(poses[t, 0] - xr[:3]).max()))
    x32, S32, _ = e.state()
    assert e.status() == 0
    e.close()
    xr, Sr, _, _ = ref.get()
    ERRORS["n1024_fp32_" + ("devsync" if env["EKF_DEVSYNC"] == "1" else "events")] = {
        "pose": err, "state": float(np.abs(x32 - xr).max()),
        "sigma": float(np.abs(S32 - Sr).max())}
    # measured (round 2): pose 2.8e-8, state 5.0e-7, Σ 1.3e-6 — bounds ≈ 20–40× above
    assert err < F32_POSE_TOL
    assert np.all(np.isfinite(S32))
    assert np.abs(x32 - xr).max() < F32_STATE_TOL
    assert np.abs(S32 - Sr).max() < F32_SIGMA_TOL


@pytest.mark.parametrize("devsync", ["1", "0"], ids=["devsync", "events"])
def test_n1024_fp32_staged_rebuild_bit_identical(n1024, devsync, monkeypatch):
    """configs[2] fp32 (the block patch the Σ pass's tiles write over their U × U entries, and
    k_stage must see it): 12 circle messages from the survey's state with the rebuild operands
    staged behind the Σ passes and gathered by the chains (EKF_STAGE=0): bit-identical."""
    sc, odom, ws = n1024
    w = sc.n_warm
    out = []
    for stage in ("1", "0"):
        for k in ("EKF_SERIAL", "EKF_CU_SPLIT", "EKF_DEVSYNC", "EKF_STAGE"):
            monkeypatch.delenv(k, raising=False)
        monkeypatch.setenv("EKF_DEVSYNC", devsync)
        monkeypatch.setenv("EKF_STAGE", stage)
        e = pyekf.EKF(n_landmarks=1024, dtype=pyekf.EKF_F32)
        x, S, tmo, cnt = ws
        e.set_state(x, S, tmo=tmo, counter=cnt)
        _replay(e, slice(w, w + 12), sc, odom)
        out.append(e.state())
        assert e.status() == 0
        e.close()
    np.testing.assert_array_equal(out[0][0], out[1][0])
    np.testing.assert_array_equal(out[0][1], out[1][1])




@pytest.mark.parametrize("dtype", [pyekf.EKF_F32, pyekf.EKF_F64], ids=["f32", "f64"])
def test_n1024_joseph_populated_against_oracle(n1024, dtype):
    """configs[2]'s populated map with the Joseph form (BASELINE.json north_star; ekf_set_joseph)
    on the HBM pipeline: 6 circle messages (96 corrections in chunks of ≤ 8, one Σ pass per chunk
    with the V_c·K_cᵀ terms folded in; host-planned, pose per message) from the fp64 survey's
    state against the oracle's Joseph mode. fp32 within the fp32 tolerances above (poses 1e-6,
    state 1e-5, Σ 5e-5), fp64 state 5e-8 and Σ 1e-7 (the populated-map tolerances above)."""
    sc, odom, ws = n1024
    w, T = sc.n_warm, 6
    e = pyekf.EKF(n_landmarks=1024, dtype=dtype)
    x, S, tmo, cnt = ws
    e.set_state(x, S, tmo=tmo, counter=cnt)
    assert e.set_joseph(True) == pyekf.EKF_OK
    poses = _replay(e, slice(w, w + T), sc, odom, poses=True)
    ref = orc.OracleEKF(n_landmarks=1024, joseph=True)
    ref.set(x, S, tmo, x[:3], cnt)
    err = 0.0
    for t in range(T):
        ref.set_odom(odom[w + t])
        c = int(sc.count[w + t])
        ref.fake_sensor_cb(sc.ids[w + t, :c], sc.actions[w + t, :c], sc.rel[w + t, :c])
        err = max(err, float(np.abs(poses[t, 0] - ref.get(sigma=False)[0][:3]).max()))
    xg, Sg, _ = e.state()
    assert e.status() == 0
    e.close()
    xr, Sr, _, _ = ref.get()
    ERRORS["n1024_joseph_" + ("f32" if dtype == pyekf.EKF_F32 else "f64")] = {
        "pose": err, "state": float(np.abs(xg - xr).max()), "sigma": float(np.abs(Sg - Sr).max())}
    if dtype == pyekf.EKF_F32:  # measured (round 2): pose 4.2e-8, Σ 1.8e-6
        assert err < F32_POSE_TOL
        assert np.all(np.isfinite(Sg))
        assert np.abs(xg - xr).max() < F32_STATE_TOL
        assert np.abs(Sg - Sr).max() < F32_SIGMA_TOL
    else:
        assert err < POSE_TOL
        assert np.abs(xg - xr).max() < STATE_TOL
        assert np.abs(Sg - Sr).max() < SIGMA_TOL


def test_swarm_n256_512_filters_against_oracle():
    """configs[3], one GPU's share: 512 filters of N=256 fp64 in one handle, filter f seeded
    base + f (its own map, slip and noise), survey + 8 circle messages. Every filter's status is
    clear and every landmark initialised; 8 strided filters equal their own oracle runs."""
    F = 512
    sw = synth.swarm(256, F, 8)
    T = sw.count.shape[0]
    odom = np.repeat(pyekf.odometry(sw.scenario(0))[:, None], F, 1)
    e = pyekf.EKF(n_landmarks=256, n_filters=F)
    e.replay(sw.count, sw.rel, odom, ids=sw.ids, actions=sw.actions)
    assert [e.status(f) for f in range(F)] == [0] * F
    init = [_initialised(e.state(f, sigma=False)[0]) for f in range(F)]
    assert min(init) == 256
    errs = []
    for f in range(0, F, F // 8):
        o = orc.run_scenario(sw.scenario(f), False)
        x, S, cnt = e.state(f)
        errs.append((float(np.abs(x - o["state"]).max()), float(np.abs(S - o["sigma"]).max())))
        assert np.abs(x[:3] - o["poses"][-1]).max() < STATE_TOL, f
        assert np.abs(x - o["state"]).max() < STATE_TOL, f
        assert np.abs(S - o["sigma"]).max() < SIGMA_TOL, f
    e.close()
    ERRORS["swarm_n256x512"] = {"state": max(a for a, _ in errs), "sigma": max(b for _, b in errs),
                                "messages": T}


@pytest.fixture(scope="module")
def known_map():
    """512 slots, 256 landmarks surveyed with known ids (fp64 pipeline): the state the unknown-
    association messages start from, counter = 256 (slam.cpp:351-356 numbering)."""
    sc = synth.populated(512, 6, n_map=256, shuffle=True)
    odom = pyekf.odometry(sc)
    e = pyekf.EKF(n_landmarks=512)
    _replay(e, slice(0, sc.n_warm), sc, odom)
    x, S, _ = e.state()
    ws = (x, S, e.map_odom(), 256)
    e.close()
    assert _initialised(x) == 256
    return sc, odom, ws


def test_association_at_scale_decisions(known_map):
    """ekf_sensor (sensor_cb) against ≥ 256 known landmarks on the pipeline: every marker's
    decision (landmark index, new or not) equal to the oracle's, poses 1e-8."""
    sc, odom, ws = known_map
    e = pyekf.EKF(n_landmarks=512)
    x, S, tmo, cnt = ws
    e.set_state(x, S, tmo=tmo, counter=cnt)
    ref = _oracle_from(ws, 512)
    n_new = n_old = 0
    for t in range(sc.n_warm, sc.n_messages):
        e.set_odom(odom[t])
        ref.set_odom(odom[t])
        c = int(sc.count[t])
        rc, j, nw = e.sensor(sc.rel[t, :c])
        rr, jr, nr = ref.sensor_cb(sc.rel[t, :c])
        assert rc == rr == 0
        assert np.array_equal(j, jr) and np.array_equal(nw, nr), t
        n_new += int(nr.sum())
        n_old += int(c - nr.sum())
        assert np.abs(e.pose() - ref.get(sigma=False)[0][:3]).max() < POSE_TOL
    xg, Sg, cg = e.state()
    xr, Sr, _, cr = ref.get()
    e.close()
    ERRORS["assoc_n512_known256"] = {"new": n_new, "associated": n_old, "counter": int(cg),
                                     "state": float(np.abs(xg - xr).max()),
                                     "sigma": float(np.abs(Sg - Sr).max())}
    assert cg == cr and cg >= 256
    assert n_old > 0  # some markers really matched known landmarks
    assert np.abs(xg - xr).max() < POSE_TOL
    assert np.abs(Sg - Sr).max() < SIGMA_TOL


def test_association_at_scale_schedules_bit_identical(known_map, monkeypatch):
    """Unknown association on the pipeline under the three schedules — device epochs (k_assoc
    polls the last Σ pass's epoch), HIP events (the main stream joins the bulk stream before each
    k_assoc) and one stream — and k_assoc_msg's two exchange transports (agent-coherent, and
    XCD-local: the filter's 8 workgroups on one XCD, EKF_AM_XCD): the same decisions and
    bit-identical state."""
    sc, odom, ws = known_map
    w = sc.n_warm
    out = []
    for env in ({"EKF_DEVSYNC": "1", "EKF_AM_XCD": "0"}, {"EKF_DEVSYNC": "0", "EKF_AM_XCD": "0"},
                {"EKF_SERIAL": "1", "EKF_AM_XCD": "0"}, {"EKF_DEVSYNC": "1", "EKF_AM_XCD": "1"},
                {"EKF_SERIAL": "1", "EKF_AM_XCD": "1"}):
        for k in ("EKF_SERIAL", "EKF_CU_SPLIT", "EKF_DEVSYNC", "EKF_AM_XCD"):
            monkeypatch.delenv(k, raising=False)
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        e = pyekf.EKF(n_landmarks=512)
        x, S, tmo, cnt = ws
        e.set_state(x, S, tmo=tmo, counter=cnt)
        _replay(e, slice(w, w + 4), sc, odom, assoc=True)
        out.append(e.state())
        assert e.status() == 0
        e.close()
    for o in out[1:]:
        assert o[2] == out[0][2]
        np.testing.assert_array_equal(o[0], out[0][0])
        np.testing.assert_array_equal(o[1], out[0][1])


@pytest.mark.parametrize("nf", [3, 9], ids=["3filters", "9filters"])
def test_association_at_scale_many_filters_xcd_placement(known_map, nf, monkeypatch):
    """k_assoc_msg with several filters: filter f's 8 workgroups are placed on XCD f mod 8 (with 9
    filters two share an XCD). The same messages to every filter from the same state, XCD-local and
    agent-coherent exchanges: every filter's state bit-identical across both and filters, equal to
    the oracle's."""
    sc, odom, ws = known_map
    w = sc.n_warm
    sl = slice(w, sc.n_messages)
    x, S, tmo, cnt = ws
    out = []
    for xcd in ("1", "0"):
        monkeypatch.setenv("EKF_AM_XCD", xcd)
        e = pyekf.EKF(n_landmarks=512, n_filters=nf)
        for f in range(nf):
            e.set_state(x, S, tmo=tmo, counter=cnt, f=f)
        T = sc.n_messages - w
        rep = lambda a: np.repeat(a[sl, None], nf, axis=1)  # noqa: E731
        e.replay(rep(sc.count), rep(sc.rel), rep(odom), ids=None, actions=rep(sc.actions),
                 assoc=True)
        assert T > 0 and all(e.status(f) == 0 for f in range(nf))
        out.append([e.state(f) for f in range(nf)])
        e.close()
    ref = _oracle_from(ws, 512)
    for t in range(w, sc.n_messages):
        ref.set_odom(odom[t])
        ref.sensor_cb(sc.rel[t, :int(sc.count[t])])
    xr, Sr, _, cr = ref.get()
    for st in out:
        for xg, Sg, cg in st:
            np.testing.assert_array_equal(xg, out[0][0][0])
            np.testing.assert_array_equal(Sg, out[0][0][1])
            assert cg == cr
    assert np.abs(out[0][0][0] - xr).max() < POSE_TOL
    assert np.abs(out[0][0][1] - Sr).max() < SIGMA_TOL


def test_association_at_scale_batched_replay(known_map):
    """The same messages through ekf_replay(assoc=1) (decisions on the device, no host round
    trip), from the same state: the final state equals the oracle's."""
    sc, odom, ws = known_map
    e = pyekf.EKF(n_landmarks=512)
    x, S, tmo, cnt = ws
    e.set_state(x, S, tmo=tmo, counter=cnt)
    w = sc.n_warm
    _replay(e, slice(w, sc.n_messages), sc, odom, assoc=True)
    ref = _oracle_from(ws, 512)
    for t in range(w, sc.n_messages):
        ref.set_odom(odom[t])
        ref.sensor_cb(sc.rel[t, :int(sc.count[t])])
    xg, Sg, cg = e.state()
    xr, Sr, _, cr = ref.get()
    assert e.status() == 0
    e.close()
    assert cg == cr
    assert np.abs(xg - xr).max() < POSE_TOL
    assert np.abs(Sg - Sr).max() < SIGMA_TOL


def _open_map_scenario():
    """512 slots, 320 landmarks. Half of the landmarks the circle messages will see are relabelled
    to the top slots and forgotten after the known-id survey, so unknown association meets both
    mapped landmarks and unmapped ones (new-landmark commits at counter ≥ 256, slam.cpp:421-422)."""
    sc = synth.populated(512, 12, n_map=320, shuffle=True)
    w = sc.n_warm
    live = np.arange(sc.ids.shape[1])[None, :] < sc.count[w:, None]
    seen = np.unique(sc.ids[w:][live])
    unmapped = seen[::2]
    mapped = np.setdiff1d(np.arange(320), unmapped)
    perm = np.empty(512, np.int32)
    perm[mapped] = np.arange(mapped.size)
    perm[unmapped] = mapped.size + np.arange(unmapped.size)
    perm[320:] = np.arange(320, 512)
    ids = np.where(sc.ids >= 0, perm[np.maximum(sc.ids, 0)], -1).astype(np.int32)
    sc = synth.Scenario(sc.n_landmarks, sc.landmarks, sc.wheel, ids, sc.actions, sc.rel,
                        sc.count, sc.truth, sc.track, sc.radius, sc.n_warm)
    return sc, int(mapped.size)


@pytest.fixture(scope="module")
def open_map():
    """The survey on the GPU (fp64), then the unmapped slots reset to the prior (slam.cpp:127-132):
    state (0, 0), no cross covariance, 1e7 on the diagonal; counter = the mapped count (≥ 256)."""
    sc, counter = _open_map_scenario()
    assert counter >= 256
    odom = pyekf.odometry(sc)
    e = pyekf.EKF(n_landmarks=512)
    _replay(e, slice(0, sc.n_warm), sc, odom)
    x, S, _ = e.state()
    tmo = e.map_odom()
    e.close()
    k = 3 + 2 * counter
    x[k:] = 0.0
    S[k:, :] = 0.0
    S[:, k:] = 0.0
    S[np.arange(k, S.shape[0]), np.arange(k, S.shape[0])] = 10e6
    return sc, odom, (x, S, tmo, counter)


def _assoc_oracle_run(sc, odom, ws, gate=2.0):
    x, S, tmo, cnt = ws
    ref = orc.OracleEKF(n_landmarks=512, mah_gate=gate)
    ref.set(x, S, tmo, x[:3], cnt)
    out = []
    for t in range(sc.n_warm, sc.n_messages):
        ref.set_odom(odom[t])
        out.append(ref.sensor_cb_dmin(sc.rel[t, :int(sc.count[t])]) + (ref.get(sigma=False)[0][:3],))
    return ref, out


def _assoc_gpu_against(sc, odom, ws, ref_out, dtype=pyekf.EKF_F64, gate=2.0):
    x, S, tmo, cnt = ws
    e = pyekf.EKF(n_landmarks=512, dtype=dtype, mah_gate=gate)
    e.set_state(x, S, tmo=tmo, counter=cnt)
    perr = 0.0
    n_new = n_old = 0
    for i, t in enumerate(range(sc.n_warm, sc.n_messages)):
        e.set_odom(odom[t])
        rc, j, nw = e.sensor(sc.rel[t, :int(sc.count[t])])
        rr, jr, nr, _, pr = ref_out[i]
        assert rc == rr == 0
        assert np.array_equal(j, jr) and np.array_equal(nw, nr), (t, j, jr, nw, nr)
        n_new += int(nr.sum())
        n_old += int(nr.size - nr.sum())
        perr = max(perr, float(np.abs(e.pose() - pr).max()))
    xg, Sg, cg = e.state()
    assert e.status() == 0
    e.close()
    return perr, xg, Sg, cg, n_new, n_old


@pytest.mark.parametrize("dtype", [pyekf.EKF_F64, pyekf.EKF_F32], ids=["f64", "f32"])
def test_association_open_map_new_and_known(open_map, dtype):
    """sensor_cb against ≥ 256 mapped landmarks with unmapped ones in view: both branches of
    slam.cpp:421-440 (commit at counter ≥ 256, roll back) with every decision equal to the
    oracle's; poses 1e-8 (fp64) / 1e-6 (fp32 Σ)."""
    sc, odom, ws = open_map
    ref, out = _assoc_oracle_run(sc, odom, ws)
    perr, xg, Sg, cg, n_new, n_old = _assoc_gpu_against(sc, odom, ws, out, dtype)
    xr, Sr, _, cr = ref.get()
    key = "assoc_open_" + ("f64" if dtype == pyekf.EKF_F64 else "f32")
    ERRORS[key] = {"new": n_new, "associated": n_old, "counter": int(cg), "pose": perr,
                   "state": float(np.abs(xg - xr).max()), "sigma": float(np.abs(Sg - Sr).max())}
    assert n_new > 0 and n_old > 0
    assert cg == cr and cr > ws[3] >= 256
    if dtype == pyekf.EKF_F64:
        assert perr < POSE_TOL
        assert np.abs(xg - xr).max() < STATE_TOL
        assert np.abs(Sg - Sr).max() < SIGMA_TOL
    else:
        assert perr < F32_POSE_TOL
        assert np.abs(xg - xr).max() < F32_STATE_TOL
        assert np.abs(Sg - Sr).max() < F32_SIGMA_TOL


def test_association_near_the_gate(open_map):
    """A gate placed 3e-4 below the first known-landmark distance in (0.5, 2): that marker's
    smallest d sits just above the gate (slam.cpp:401-408; the new slot, index counter, wins only
    over a strictly larger existing minimum), every earlier decision unchanged. Every decision,
    the near-gate one included, equals the oracle's."""
    sc, odom, ws = open_map
    _, out = _assoc_oracle_run(sc, odom, ws)
    d = np.concatenate([o[3] for o in out])
    i0 = int(np.argmax((d > 0.5) & (d < 2.0)))
    assert 0.5 < d[i0] < 2.0
    gate = float(d[i0]) - 3e-4
    ref, out = _assoc_oracle_run(sc, odom, ws, gate)
    d2 = np.concatenate([o[3] for o in out])
    near = np.flatnonzero(np.abs(d2 - gate) < 1e-3)
    assert near.size > 0 and i0 in near
    perr, xg, Sg, cg, n_new, n_old = _assoc_gpu_against(sc, odom, ws, out, gate=gate)
    xr, Sr, _, cr = ref.get()
    ERRORS["assoc_near_gate"] = {"gate": gate, "near": near.tolist(), "new": n_new,
                                 "associated": n_old, "pose": perr,
                                 "state": float(np.abs(xg - xr).max())}
    assert cg == cr
    assert perr < POSE_TOL
    assert np.abs(xg - xr).max() < STATE_TOL
    assert np.abs(Sg - Sr).max() < SIGMA_TOL
