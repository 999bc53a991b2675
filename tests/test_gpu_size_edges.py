"""The Σ pass, the factor kernel and the association kernel at tile and workgroup edges.

n = 3 + 2N. Every pipeline size the rest of the suite runs has n mod 32 in {3, 7}; the sizes here
give n mod 32 = 31, 1, 15, 17 (a last 32x32 / 16x16 / 32x64 tile row and column 31, 1, 15 or 17
elements wide, ld = n + 1 or n rounded up, the buffer-descriptor range check in place of masks),
with N = 64 (n = 131, residue 3) as the control, on populated maps: every landmark is initialised,
so the last rows and columns are live. N = 110 (n = 223, 7 × 7 tiles of 32 × 32) is the last size
on the Σ pass's plain grid, N = 111 (n = 225, 8 × 8 tiles, the last ones one element wide) the
first on its XCD-region grid (sigma_grid.hpp). k_assoc_msg puts 64 slots in a workgroup: N = 63, 65, 127,
129 leave 63, 1, 63, 1 live lanes in the last one, with a commit on the very last slot.

Bounds are test_gpu_scale.py's, whose docstring derives them for exactly this kind of surveyed map
(these maps have fewer first sightings than its N = 256): fp64 pose 1e-8, state 5e-8, Σ 1e-7; fp32
Σ 5e-6 / 1e-5 / 5e-5. A size that exceeds a bound while the N = 64 control stays inside is an edge
bug in the kernel. Measured errors are merged into edge_errors.json (beside
scale_errors.json).
"""
import numpy as np
import pytest

import edge_scenarios as es
import orc
import pyekf
from pyekf import synth

pytestmark = pytest.mark.gpu

F64_TOL = es.ASSOC_TOL   # 1e-8 / 5e-8 / 1e-7, test_gpu_scale.py's populated-map bounds
F32_TOL = es.F32_TOL     # 5e-6 / 1e-5 / 5e-5, its N = 256 survey test's
KNOWN_SIZES = [14, 15, 31, 63, 64, 70, 71, 78, 79, 94, 95, 110, 111, 127]
WIDE_SIZES = [15, 63, 78, 94, 95]
ASSOC_SIZES = [63, 65, 127, 129]
ERRORS = {}
RANGE = pyekf.EKF_FLAG_RANGE


@pytest.fixture(scope="module", autouse=True)
def _record_errors():
    yield
    es.write_errors("size_edges", ERRORS)


@pytest.fixture(autouse=True)
def _pipeline(monkeypatch):
    for k in ("EKF_SERIAL", "EKF_CU_SPLIT", "EKF_DEVSYNC", "EKF_STAGE", "EKF_ASSOC_MSG",
              "EKF_AM_XCD"):
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("EKF_RESIDENT", "0")


def _initialised(x):
    return int(np.count_nonzero(np.any(x[3:].reshape(-1, 2) != 0.0, 1)))


def _dt(dtype):
    return "f64" if dtype == pyekf.EKF_F64 else "f32"


_cache: dict = {}


def _known(N):
    """populated(N, 6) and its odometry, once per module."""
    if ("sc", N) not in _cache:
        sc = synth.populated(N, 6)
        _cache["sc", N] = (sc, pyekf.odometry(sc))
    return _cache["sc", N]


def _known_oracle(N, joseph):
    if ("ref", N, joseph) not in _cache:
        sc, odom = _known(N)
        ref = orc.OracleEKF(n_landmarks=N, joseph=joseph)
        for t in range(sc.n_messages):
            ref.set_odom(odom[t])
            c = int(sc.count[t])
            assert ref.fake_sensor_cb(sc.ids[t, :c], sc.actions[t, :c], sc.rel[t, :c]) == 0
        _cache["ref", N, joseph] = ref.get()
    return _cache["ref", N, joseph]


@pytest.mark.parametrize("joseph", [False, True], ids=["simple", "joseph"])
@pytest.mark.parametrize("dtype", [pyekf.EKF_F64, pyekf.EKF_F32], ids=["f64", "f32"])
@pytest.mark.parametrize("N", KNOWN_SIZES)
def test_known_ids_at_tile_edges(N, dtype, joseph):
    """Survey + 6 circle messages in one ekf_replay upload on the pipeline, against the oracle in
    the same form."""
    sc, odom = _known(N)
    xr, Sr, tmr, cr = _known_oracle(N, joseph)
    e = pyekf.EKF(n_landmarks=N, dtype=dtype)
    assert e.path == pyekf.EKF_PATH_PIPELINE and e.n == 3 + 2 * N
    assert e.set_joseph(joseph) == pyekf.EKF_OK
    e.replay(sc.count[:, None], sc.rel[:, None], odom[:, None], ids=sc.ids[:, None],
             actions=sc.actions[:, None])
    x, S, cnt = e.state()
    tmo = e.map_odom()
    assert e.status() == 0
    e.close()
    assert cnt == cr and _initialised(x) == N and _initialised(xr) == N
    err = {"n": 3 + 2 * N, "messages": sc.n_messages,
           "pose": float(np.abs(x[:3] - xr[:3]).max()), "state": float(np.abs(x - xr).max()),
           "sigma": float(np.abs(S - Sr).max()), "tmo": float(np.abs(tmo - tmr).max())}
    ERRORS[f"known/N{N}/{_dt(dtype)}/{'joseph' if joseph else 'simple'}"] = err
    pt, st, sg = F64_TOL if dtype == pyekf.EKF_F64 else F32_TOL
    assert np.all(np.isfinite(S))
    assert err["pose"] < pt, err
    assert err["tmo"] < st, err
    assert err["state"] < st, err
    assert err["sigma"] < sg, err
    if dtype == pyekf.EKF_F64:   # the symmetric fp64 pass mirrors its upper triangle
        np.testing.assert_array_equal(S, S.T)


@pytest.mark.parametrize("N", WIDE_SIZES)
def test_wide_tiles_sixteen_filters(N):
    """16 filters (the wide 32x64 fp64 tile and the XCD-aware grid), each with its own map: every
    status 0, every landmark initialised, Σ exactly symmetric; four strided filters against their
    oracle runs."""
    F = 16
    sw = synth.swarm(N, F, 6)
    odom = np.repeat(pyekf.odometry(sw.scenario(0))[:, None], F, 1)
    e = pyekf.EKF(n_landmarks=N, n_filters=F)
    assert e.path == pyekf.EKF_PATH_PIPELINE
    e.replay(sw.count, sw.rel, odom, ids=sw.ids, actions=sw.actions)
    assert [e.status(f) for f in range(F)] == [0] * F
    worst = {"pose": 0.0, "state": 0.0, "sigma": 0.0}
    for f in range(F):
        x, S, _ = e.state(f)
        assert _initialised(x) == N, f
        np.testing.assert_array_equal(S, S.T)
        if f % 4 == 1:
            o = orc.run_scenario(sw.scenario(f), False)
            es_, ss_ = float(np.abs(x - o["state"]).max()), float(np.abs(S - o["sigma"]).max())
            ps_ = float(np.abs(x[:3] - o["poses"][-1]).max())
            worst = {"pose": max(worst["pose"], ps_), "state": max(worst["state"], es_),
                     "sigma": max(worst["sigma"], ss_)}
            assert ps_ < F64_TOL[0], (f, ps_)
            assert es_ < F64_TOL[1], (f, es_)
            assert ss_ < F64_TOL[2], (f, ss_)
    e.close()
    ERRORS[f"wide/N{N}x16"] = dict(worst, n=3 + 2 * N, messages=int(sw.count.shape[0]))


# ---- association at workgroup edges -----------------------------------------------------------------
def _assoc_map(N, variant):
    """populated(N, 6, shuffle=True) surveyed with known ids on the GPU (fp64 pipeline) → the
    scenario, its odometry and the state (x, S, tmo, counter) the unknown-association circle
    messages start from.

    full: counter = N, every slot mapped (each marker then meets a full map: slam.cpp:351 indexes
    past the state; EKF_E_RANGE). last: a landmark the circle messages see (es.LAST_SLOT) is
    relabelled to slot N - 1, that slot is reset to the prior (slam.cpp:127-132) and
    counter = N - 1: markers associate against N - 1 landmarks until that one is sighted and
    committed on the very last slot — the last live lane of k_assoc_msg's last workgroup."""
    if (N, variant) in _cache:
        return _cache[N, variant]
    sc = synth.populated(N, 6, shuffle=True)
    w = sc.n_warm
    counter = N
    if variant == "last":
        sc = es.last_slot_scenario(N)
        counter = N - 1
    odom = pyekf.odometry(sc)
    e = pyekf.EKF(n_landmarks=N)
    assert e.path == pyekf.EKF_PATH_PIPELINE
    e.replay(sc.count[:w, None], sc.rel[:w, None], odom[:w, None], ids=sc.ids[:w, None],
             actions=sc.actions[:w, None])
    x, S, _ = e.state()
    tmo = e.map_odom()
    assert e.status() == 0
    e.close()
    assert _initialised(x) == N
    if variant == "last":
        es.forget_last(x, S)
    _cache[N, variant] = (sc, odom, (x, S, tmo, counter))
    return _cache[N, variant]


@pytest.mark.parametrize("dtype", [pyekf.EKF_F64, pyekf.EKF_F32], ids=["f64", "f32"])
@pytest.mark.parametrize("variant", ["full", "last"])
@pytest.mark.parametrize("N", ASSOC_SIZES)
def test_association_at_workgroup_edges(N, variant, dtype):
    """ekf_sensor with decisions from the surveyed map: every decision and the counter equal the
    oracle's; EKF_E_RANGE and EKF_FLAG_RANGE appear exactly where the oracle returns -2."""
    sc, odom, ws = _assoc_map(N, variant)
    x0, S0, tmo0, cnt0 = ws
    e = pyekf.EKF(n_landmarks=N, dtype=dtype)
    assert e.path == pyekf.EKF_PATH_PIPELINE
    assert e.assoc_route in (pyekf.EKF_ASSOC_CHUNK, pyekf.EKF_ASSOC_CHUNK_XCD)
    e.set_state(x0, S0, tmo=tmo0, counter=cnt0)
    ref = orc.OracleEKF(n_landmarks=N)
    ref.set(x0, S0, tmo0, x0[:3], cnt0)
    perr, n_old, commits, rcs = 0.0, 0, [], []
    for t in range(sc.n_warm, sc.n_messages):
        c = int(sc.count[t])
        e.set_odom(odom[t])
        ref.set_odom(odom[t])
        rc, j, nw = e.sensor(sc.rel[t, :c])
        rr, jr, nr, dmin = ref.sensor_cb_dmin(sc.rel[t, :c])
        d = dmin[np.isfinite(dmin)]
        assert d.size == 0 or np.abs(d - 2.0).min() >= 0.05   # no decision near the gate
        assert rr in (0, -2) and rc == rr, (t, rc, rr)
        assert np.array_equal(j, jr) and np.array_equal(nw, nr), (t, j, jr, nw, nr)
        assert e.status() == (RANGE if rr == -2 else 0), t
        xr, _, _, cr = ref.get(sigma=False)
        assert e.state(sigma=False)[2] == cr
        perr = max(perr, float(np.abs(e.pose() - xr[:3]).max()))
        n_old += int(np.count_nonzero((jr >= 0) & (nr == 0)))
        commits += [int(a) for a in jr[nr == 1]]
        rcs.append(int(rr))
    xg, Sg, cg = e.state()
    e.close()
    xr, Sr, _, cr = ref.get()
    if variant == "full":   # no marker can be placed: predict and posterior only
        assert rcs == [-2] * len(rcs) and n_old == 0 and commits == []
    else:                   # the one commit landed on the last slot (and the map is full after it)
        assert commits == [N - 1] and n_old > 0
        assert np.any(xg[3 + 2 * (N - 1):] != 0.0)
    err = {"pose": perr, "state": float(np.abs(xg - xr).max()),
           "sigma": float(np.abs(Sg - Sr).max()), "associated": n_old}
    ERRORS[f"assoc/N{N}/{variant}/{_dt(dtype)}"] = err
    pt, st, sg = F64_TOL if dtype == pyekf.EKF_F64 else F32_TOL
    assert cg == cr == N
    assert err["pose"] < pt, err
    assert err["state"] < st, err
    assert err["sigma"] < sg, err
