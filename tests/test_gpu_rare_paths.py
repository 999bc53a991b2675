"""The correction kernels' generic paths on the GPU, against the oracle.

Every scenario of tests/edge_scenarios.py (pinned by tests/test_edge_scenarios.py) goes through
the product: a skipped marker (range-0 first sighting: S is NaN, EKF_FLAG_NUMERIC, the oracle's
-4) whose zeroed H / S^-1 / innovation / K and M columns the chain's other waves, the factor kernel,
the Σ pass, the next chunk's rebuild and the fp32 block patch consume; headings far outside
(-pi, pi]; bearings and a heading on the +-pi seam; a range-0 marker under unknown association.
Resident path, fp64 and fp32 pipeline, simple and Joseph form, every submission form and schedule,
several filters in one handle, every association route.

Bounds (edge_scenarios.KNOWN_TOL / ASSOC_TOL / F32_TOL) are the suite's own: fp64 known-id 1e-8
(test_gpu_parity.py); fp64 association 1e-8 / 5e-8 / 1e-7 and fp32 5e-6 / 1e-5 / 5e-5 (pose /
state / Σ, test_gpu_scale.py). Decisions, counters and status flags are exact. Measured maxima go
to edge_errors.json, beside test_gpu_scale.py's scale_errors.json.
"""
import numpy as np
import pytest

import edge_scenarios as es
import orc
import pyekf

pytestmark = pytest.mark.gpu

NUMERIC = pyekf.EKF_FLAG_NUMERIC
ERRORS = {}
ENV_KEYS = ("EKF_RESIDENT", "EKF_SERIAL", "EKF_CU_SPLIT", "EKF_DEVSYNC", "EKF_STAGE",
            "EKF_ASSOC_MSG", "EKF_AM_XCD")
# path id → (environment, dtype, the path the handle must report)
PATHS = {
    "resident": ({}, pyekf.EKF_F64, pyekf.EKF_PATH_RESIDENT),
    "pipe64": ({"EKF_RESIDENT": "0"}, pyekf.EKF_F64, pyekf.EKF_PATH_PIPELINE),
    "pipe32": ({}, pyekf.EKF_F32, pyekf.EKF_PATH_PIPELINE),
}
FORMS = pytest.mark.parametrize("joseph", [False, True], ids=["simple", "joseph"])


@pytest.fixture(scope="module", autouse=True)
def _record_errors():
    yield
    es.write_errors("rare_paths", ERRORS)


def _env(monkeypatch, env):
    for k in ENV_KEYS:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


_oracle: dict = {}


def _ref(name, joseph):
    """The structured oracle's run of a scenario, once per module."""
    if (name, joseph) not in _oracle:
        _oracle[name, joseph] = es.run_oracle(es.get(name), joseph=joseph)
    return _oracle[name, joseph]


def _handle(e, dtype, joseph, path=None, F=1):
    h = pyekf.EKF(n_landmarks=e.n_landmarks, n_filters=F, dtype=dtype)
    if path is not None:
        assert h.path == path
    assert h.set_joseph(joseph) == pyekf.EKF_OK
    return h


def _arrays(edges):
    """ekf_replay's arrays [T][F](...) for one scenario per filter (same T)."""
    T, F = edges[0].n_messages, len(edges)
    M = max(e.ids.shape[1] for e in edges)
    cnt = np.zeros((T, F), np.int32)
    ids = np.zeros((T, F, M), np.int32)
    act = np.zeros((T, F, M), np.int32)
    rel = np.zeros((T, F, M, 2))
    od = np.zeros((T, F, 3))
    for f, e in enumerate(edges):
        m = e.ids.shape[1]
        cnt[:, f] = e.count
        ids[:, f, :m] = np.maximum(e.ids, 0)
        act[:, f, :m] = e.actions
        rel[:, f, :m] = e.rel
        od[:, f] = e.odom
    return cnt, ids, act, rel, od


def _flag(rc):
    return NUMERIC if rc == es.NUMERIC else 0


def _submit(h, e, how, ref):
    """Every message of a known-id scenario through one submission form; the status is read per
    message on the per-message forms, once after a replay, and must be EKF_FLAG_NUMERIC exactly
    where the oracle returned -4 and 0 elsewhere. → the worst pose error of the per-message forms
    (None for the replays)."""
    T = e.n_messages
    perr = None
    if how in ("sensor", "fine"):
        perr = 0.0
        for t in range(T):
            c = int(e.count[t])
            assert h.set_odom(e.odom[t]) == 0
            if how == "sensor":  # asynchronous: a skip is reported through the flag only
                assert h.fake_sensor(e.ids[t, :c], e.actions[t, :c], e.rel[t, :c]) == 0
            else:
                assert h.predict() == 0
                for i in range(c):
                    assert h.correct(e.ids[t, i], *e.rel[t, i]) == 0
                assert h.posterior() == 0
            assert h.status() == _flag(ref["rcs"][t]), t
            perr = max(perr, float(np.abs(h.pose() - ref["poses"][t]).max()))
    elif how == "replay":
        cnt, ids, act, rel, od = _arrays([e])
        h.replay(cnt, rel, od, ids=ids, actions=act)
        assert h.status() == (NUMERIC if e.skips else 0)
    elif how == "device":
        import torch
        g = [torch.from_numpy(a).cuda() for a in _arrays([e])]
        h.replay_device(g[0], g[3], g[4], g[1], g[2])
        assert h.status() == (NUMERIC if e.skips else 0)  # (synchronises: the tensors may go)
    else:
        raise ValueError(how)
    assert h.status() == 0  # cleared by the read
    return perr


def _compare(key, h, ref, tol, perr=None, f=0):
    x, S, cnt = h.state(f)
    assert np.all(np.isfinite(x)) and np.all(np.isfinite(S))
    err = {"pose": float(np.abs(x[:3] - ref["state"][:3]).max()) if perr is None else
           max(perr, float(np.abs(x[:3] - ref["state"][:3]).max())),
           "state": float(np.abs(x - ref["state"]).max()),
           "sigma": float(np.abs(S - ref["sigma"]).max()),
           "tmo": float(np.abs(h.map_odom(f) - ref["tmo"]).max())}
    ERRORS[key] = err
    assert cnt == ref["counter"]
    assert err["pose"] < tol[0], err
    assert err["tmo"] < tol[1], err
    assert err["state"] < tol[1], err
    assert err["sigma"] < tol[2], err
    return x, S


def _tol(dtype, assoc=False):
    if dtype == pyekf.EKF_F32:
        return es.F32_TOL
    return es.ASSOC_TOL if assoc else es.KNOWN_TOL


# ---- Z, H, S: every path and form, one replay upload ----------------------------------------------
@FORMS
@pytest.mark.parametrize("path", list(PATHS))
@pytest.mark.parametrize("name", list(es.KNOWN))
def test_replay_against_oracle(monkeypatch, name, path, joseph):
    """One ekf_replay upload: the persistent chain walks the chunks, and the chunk after a skipped
    marker rebuilds from a record with zero K / M columns. LDS is poisoned first."""
    env, dtype, want = PATHS[path]
    _env(monkeypatch, env)
    e, ref = es.get(name), _ref(name, joseph)
    pyekf.poison_lds()
    h = _handle(e, dtype, joseph, want)
    _submit(h, e, "replay", ref)
    _compare(f"replay/{name}/{path}/{'joseph' if joseph else 'simple'}", h, ref, _tol(dtype))
    h.close()


# ---- Z, H (and S): the per-message forms ----------------------------------------------------------
@FORMS
@pytest.mark.parametrize("how", ["sensor", "fine"])
@pytest.mark.parametrize("path", list(PATHS))
@pytest.mark.parametrize("name", list(es.KNOWN))
def test_per_message_forms_against_oracle(monkeypatch, name, path, how, joseph):
    """ekf_fake_sensor per message, and ekf_predict / ekf_correct / ekf_posterior (one chunk per
    marker): the status flag message by message, every posterior pose, the final state."""
    env, dtype, want = PATHS[path]
    _env(monkeypatch, env)
    e, ref = es.get(name), _ref(name, joseph)
    h = _handle(e, dtype, joseph, want)
    perr = _submit(h, e, how, ref)
    _compare(f"{how}/{name}/{path}/{'joseph' if joseph else 'simple'}", h, ref, _tol(dtype), perr)
    h.close()


@FORMS
@pytest.mark.parametrize("dtype", [pyekf.EKF_F64, pyekf.EKF_F32], ids=["f64", "f32"])
@pytest.mark.parametrize("name", [n for n in es.KNOWN if not n.startswith("Z20_")])
def test_device_replay_against_oracle(monkeypatch, name, dtype, joseph):
    """ekf_replay_device: the device planner forms range and bearing of rel = (0, 0) itself
    (m_max <= EKF_MAX_CHUNK: the 20-marker scenarios cannot take this form)."""
    _env(monkeypatch, {"EKF_RESIDENT": "0"})
    e, ref = es.get(name), _ref(name, joseph)
    h = _handle(e, dtype, joseph, pyekf.EKF_PATH_PIPELINE)
    _submit(h, e, "device", ref)
    _compare(f"device/{name}/{'f64' if dtype == pyekf.EKF_F64 else 'f32'}/"
             f"{'joseph' if joseph else 'simple'}", h, ref, _tol(dtype))
    h.close()


# ---- schedules ------------------------------------------------------------------------------------
@FORMS
@pytest.mark.parametrize("dtype", [pyekf.EKF_F64, pyekf.EKF_F32], ids=["f64", "f32"])
@pytest.mark.parametrize("name", ["Z12_p3", "Z16_p15", "Z20_p15", "Z20_p16", "H_p20",
                                  "Z12_p3_p20", "S_seam"])
def test_schedules_bit_identical(monkeypatch, name, dtype, joseph):
    """The default schedule, HIP events, one stream, and the chains gathering their own rebuild
    operands (EKF_STAGE=0): bit-identical on these inputs too."""
    e, ref = es.get(name), _ref(name, joseph)
    out = []
    for env in ({}, {"EKF_DEVSYNC": "0"}, {"EKF_SERIAL": "1"}, {"EKF_STAGE": "0"}):
        _env(monkeypatch, dict(env, EKF_RESIDENT="0"))
        pyekf.poison_lds()
        h = _handle(e, dtype, joseph, pyekf.EKF_PATH_PIPELINE)
        _submit(h, e, "replay", ref)
        out.append(h.state())
        h.close()
    for x, S, c in out[1:]:
        assert c == out[0][2]
        np.testing.assert_array_equal(x, out[0][0])
        np.testing.assert_array_equal(S, out[0][1])


# ---- several filters in one handle ----------------------------------------------------------------
@FORMS
@pytest.mark.parametrize("path", list(PATHS))
def test_three_filters_keep_to_themselves(monkeypatch, path, joseph):
    """F = 3: the clean base, Z(p = 3) and H(+20) side by side. Filter 0 is bit-identical to the
    clean single-filter run (a neighbour's skip or generic path touches nothing of it); filters 1
    and 2 match their own oracle runs; the status is 0, NUMERIC, 0."""
    env, dtype, want = PATHS[path]
    _env(monkeypatch, env)
    names = ["clean", "Z12_p3", "H_p20"]
    edges = [es.get(n) for n in names]
    cnt, ids, act, rel, od = _arrays(edges)
    h = _handle(edges[0], dtype, joseph, want, F=3)
    h.replay(cnt, rel, od, ids=ids, actions=act)
    assert [h.status(f) for f in range(3)] == [0, NUMERIC, 0]
    form = "joseph" if joseph else "simple"
    got = [_compare(f"filters3/{n}/{path}/{form}", h, _ref(n, joseph), _tol(dtype), f=f)
           for f, n in enumerate(names)]
    h.close()
    one = _handle(edges[0], dtype, joseph, want)
    _submit(one, edges[0], "replay", _ref("clean", joseph))
    x, S, _ = one.state()
    one.close()
    np.testing.assert_array_equal(got[0][0], x)
    np.testing.assert_array_equal(got[0][1], S)


# ---- A: unknown association -----------------------------------------------------------------------
# route id → (N, environment, resident?, the route the handle must report)
ROUTES = {
    "resident": (20, {}, True, pyekf.EKF_ASSOC_MARKER),
    "marker": (20, {"EKF_RESIDENT": "0", "EKF_ASSOC_MSG": "0"}, False, pyekf.EKF_ASSOC_MARKER),
    "chunk_1wg": (20, {"EKF_RESIDENT": "0", "EKF_AM_XCD": "0"}, False, pyekf.EKF_ASSOC_CHUNK),
    "chunk_3wg_xcd": (130, {"EKF_AM_XCD": "1"}, False, pyekf.EKF_ASSOC_CHUNK_XCD),
    "chunk_3wg_agent": (130, {"EKF_AM_XCD": "0"}, False, pyekf.EKF_ASSOC_CHUNK),
}
A_CASES = [(r, n, d) for r, (N, _, res, _) in ROUTES.items()
           for n in list(es.ASSOC) + list(es.ASSOC_MULTI) if n.startswith(f"A{N}_")
           for d in (("f64",) if res else ("f64", "f32"))]


def _assoc_handle(monkeypatch, route, e, dtype, joseph):
    N, env, res, want = ROUTES[route]
    _env(monkeypatch, env)
    h = _handle(e, pyekf.EKF_F64 if dtype == "f64" else pyekf.EKF_F32, joseph,
                pyekf.EKF_PATH_RESIDENT if res else pyekf.EKF_PATH_PIPELINE)
    assert h.assoc_route == want
    return h


@FORMS
@pytest.mark.parametrize("route,name,dtype", A_CASES)
def test_assoc_sensor_against_oracle(monkeypatch, route, name, dtype, joseph):
    """ekf_sensor with decision outputs, message by message: every decision and the counter equal
    the oracle's, the return code is the oracle's (EKF_E_NUMERIC for the message with the range-0
    marker), the status flag goes with it."""
    e, ref = es.get(name), _ref(name, joseph)
    h = _assoc_handle(monkeypatch, route, e, dtype, joseph)
    perr = 0.0
    for t in range(e.n_messages):
        c = int(e.count[t])
        h.set_odom(e.odom[t])
        rc, j, nw = h.sensor(e.rel[t, :c])
        assert rc == ref["rcs"][t], t
        assert np.array_equal(j, ref["assoc_j"][t, :c]), (t, j, ref["assoc_j"][t, :c])
        assert np.array_equal(nw, ref["assoc_new"][t, :c]), t
        assert h.status() == _flag(ref["rcs"][t]), t
        assert h.state(sigma=False)[2] == ref["counters"][t]
        perr = max(perr, float(np.abs(h.pose() - ref["poses"][t]).max()))
    tol = _tol(pyekf.EKF_F64 if dtype == "f64" else pyekf.EKF_F32, assoc=True)
    _compare(f"assoc_sensor/{name}/{route}/{dtype}/{'joseph' if joseph else 'simple'}", h, ref,
             tol, perr)
    h.close()


@FORMS
@pytest.mark.parametrize("route,name,dtype", A_CASES)
def test_assoc_replay_against_oracle(monkeypatch, route, name, dtype, joseph):
    """The same messages in one ekf_replay(assoc=1) upload (decisions on the device): the final
    state and counter, EKF_FLAG_NUMERIC and nothing else in the status."""
    e, ref = es.get(name), _ref(name, joseph)
    h = _assoc_handle(monkeypatch, route, e, dtype, joseph)
    cnt, _, act, rel, od = _arrays([e])
    h.replay(cnt, rel, od, ids=None, actions=act, assoc=True)
    assert h.status() == NUMERIC
    tol = _tol(pyekf.EKF_F64 if dtype == "f64" else pyekf.EKF_F32, assoc=True)
    _compare(f"assoc_replay/{name}/{route}/{dtype}/{'joseph' if joseph else 'simple'}", h, ref,
             tol)
    h.close()


@pytest.mark.parametrize("route,name", [("resident", "A20_3"), ("marker", "A20_3"),
                                        ("chunk_1wg", "A20_3"), ("chunk_3wg_xcd", "A130_3")])
def test_assoc_fine_grained_return_codes(monkeypatch, route, name):
    """ekf_predict / ekf_associate_correct / ekf_posterior: the marker at range 0 returns
    EKF_E_NUMERIC (the oracle's -4) and is_new = 1, the markers after it return 0 again, one of
    them associated with the phantom."""
    e = es.get(name)
    ref = orc.OracleEKF(n_landmarks=e.n_landmarks)
    h = _assoc_handle(monkeypatch, route, e, "f64", False)
    seen = []
    for t in range(e.n_messages):
        h.set_odom(e.odom[t])
        ref.set_odom(e.odom[t])
        assert h.predict() == 0
        ref.predict()
        for i in range(int(e.count[t])):
            rc, j, nw = h.associate_correct(*e.rel[t, i])
            jr, nr = orc.C.c_int(-1), orc.C.c_int(0)
            rr = orc.lib().orc_ekf_associate_correct(ref.h, float(e.rel[t, i, 0]),
                                                     float(e.rel[t, i, 1]), orc.C.byref(jr),
                                                     orc.C.byref(nr))
            assert (rc, j, nw) == (rr, jr.value, nr.value), (t, i)
            seen.append(rc)
        assert h.posterior() == 0
        ref.posterior()
    assert seen.count(pyekf.EKF_E_NUMERIC) == 1 and seen[-1] == 0
    assert h.status() == NUMERIC
    xr, Sr, tmr, cr = ref.get()
    _compare(f"assoc_fine/{name}/{route}", h,
             dict(state=xr, sigma=Sr, tmo=tmr, counter=cr), es.ASSOC_TOL)
    h.close()


@pytest.mark.parametrize("route", [r for r, v in ROUTES.items() if v[0] == 20])
def test_sync_return_codes_count_every_skip(monkeypatch, route):
    """No status read between the calls. ekf_sensor with outputs returns EKF_E_NUMERIC for each of
    two consecutive messages that skip a marker (the device's flag is already set when the second
    one skips); a skip of an asynchronous ekf_sensor (no outputs) is not charged to the
    synchronous call after it, which skipped nothing; ekf_associate_correct returns it for both
    range-0 markers of one message and 0 for the markers between. The flag shows in the status
    read that ends each run, once."""
    T = es.get("A20_two_msgs").n_messages
    for name, quiet in (("A20_two_msgs", ()), ("A20_zero_then_clean", (T - 2,))):
        e, ref = es.get(name), _ref(name, False)
        h = _assoc_handle(monkeypatch, route, e, "f64", False)
        for t in range(T):
            c = int(e.count[t])
            h.set_odom(e.odom[t])
            rc, j, nw = h.sensor(e.rel[t, :c], decisions=t not in quiet)
            if t in quiet:
                assert rc == 0
                continue
            assert rc == ref["rcs"][t], (name, t)
            assert np.array_equal(j, ref["assoc_j"][t, :c]), (name, t)
            assert np.array_equal(nw, ref["assoc_new"][t, :c]), (name, t)
        assert h.status() == NUMERIC and h.status() == 0
        _compare(f"sync_rc/{name}/{route}", h, ref, es.ASSOC_TOL)
        h.close()
    e = es.get("A20_two_same")
    ref = orc.OracleEKF(n_landmarks=e.n_landmarks)
    h = _assoc_handle(monkeypatch, route, e, "f64", False)
    seen = []
    for t in range(T):
        h.set_odom(e.odom[t])
        ref.set_odom(e.odom[t])
        assert h.predict() == 0
        ref.predict()
        for i in range(int(e.count[t])):
            rc, j, nw = h.associate_correct(*e.rel[t, i])
            jr, nr = orc.C.c_int(-1), orc.C.c_int(0)
            rr = orc.lib().orc_ekf_associate_correct(ref.h, float(e.rel[t, i, 0]),
                                                     float(e.rel[t, i, 1]), orc.C.byref(jr),
                                                     orc.C.byref(nr))
            assert (rc, j, nw) == (rr, jr.value, nr.value), (t, i)
            seen.append(rc)
        assert h.posterior() == 0
        ref.posterior()
    assert seen.count(pyekf.EKF_E_NUMERIC) == 2 and seen[-1] == pyekf.EKF_E_NUMERIC
    assert h.status() == NUMERIC and h.status() == 0
    xr, Sr, tmr, cr = ref.get()
    _compare(f"sync_rc/A20_two_same/{route}", h,
             dict(state=xr, sigma=Sr, tmo=tmr, counter=cr), es.ASSOC_TOL)
    h.close()


# ---- H without a predict: the chain's own angle fallbacks -----------------------------------------
@FORMS
@pytest.mark.parametrize("turns", [5, -5])
@pytest.mark.parametrize("path", list(PATHS))
def test_set_state_heading_without_predict(monkeypatch, path, turns, joseph):
    """ekf_set_state with a heading of about +-31 rad, then ekf_correct per marker with no predict
    pending and ekf_posterior: the first correction's bearing and updated heading lie beyond the
    branch-free normalisation's range, so the correction kernel's generic bearing and heading
    fallbacks run; the pose after every correction and the final state against the oracle loaded
    with the same state (orc set + correct). (Without the heading fallback the heading would come
    back into (-pi, pi] only after three corrections, and the final state would not show it.)"""
    env, dtype, want = PATHS[path]
    _env(monkeypatch, env)
    hs = es.heading_state(turns)
    x0, S0, tmo0, od, ids, rel = hs
    xr, Sr, tmr, pr = es.run_heading_state(hs, joseph=joseph)
    h = _handle(es.get("clean"), dtype, joseph, want)
    h.set_state(x0, S0, tmo=tmo0, counter=0)
    assert h.set_odom(od) == 0
    perr = 0.0
    for i, (lid, (rx, ry)) in enumerate(zip(ids, rel)):
        assert h.correct(lid, rx, ry) == 0
        p = h.pose()   # the heading is wrapped by the correction that met it (slam.cpp:267)
        assert abs(p[0]) <= np.pi, i
        perr = max(perr, float(np.abs(p - pr[i]).max()))
    assert h.posterior() == 0
    assert h.status() == 0
    _compare(f"set_state_heading/{turns:+d}/{path}/{'joseph' if joseph else 'simple'}", h,
             dict(state=xr, sigma=Sr, tmo=tmr, counter=0), _tol(dtype), perr)
    h.close()
