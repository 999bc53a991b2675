"""The filter's noise parameters and landmark prior away from their defaults, on the GPU against
the oracle at the same parameters.

Every other GPU test runs at ekf_config's defaults, q_noise == r_noise == 1e-2 and init_var = 1e7,
where a kernel that reads r for q, or a literal left behind by a refactor, computes the same thing.
The cases of tests/param_cases.py (pinned by tests/test_param_cases.py: well conditioned, common
case only, and at least 1e-4 away from the same run with q and r exchanged or at their defaults)
go through every site that takes a parameter:

* the resident path (k_resident per message and per host-planned replay, k_resident_replay from
  device inputs), known ids and association;
* the fp64 and the fp32 pipeline (EKF_RESIDENT=0 below N = 128): the predict's pose block in
  k_factors, the Σ pass and k_stage, the chain's fold and rebuild and its wave-0 steps, the lean
  wave-0 program (EKF_CHAIN_FAST=1), k_assoc_msg with one and with three workgroups and both
  exchange placements, k_assoc (EKF_ASSOC_MSG=0), host- and device-planned replays, the chains
  gathering their own operands (EKF_STAGE=0), one stream (EKF_SERIAL=1);
* a swarm of three filters, Σ₀ after ekf_create and ekf_reset, slam_create's configuration.

Bounds are the suite's own (edge_scenarios.KNOWN_TOL / ASSOC_TOL / F32_TOL); decisions and
counters are exact. An fp32 case starts from the fp64 state after param_cases.WARM messages
(ekf_set_state, as tests/test_gpu_scale.py); with init_var <= 1e3 it also runs from message 0.
Measured errors go to edge_errors.json, section "params".
"""
import numpy as np
import pytest

import edge_scenarios as es
import orc
import param_cases as pc
import pyekf

pytestmark = pytest.mark.gpu

ERRORS = {}
ENV_KEYS = ("EKF_RESIDENT", "EKF_SERIAL", "EKF_CU_SPLIT", "EKF_DEVSYNC", "EKF_STAGE",
            "EKF_ASSOC_MSG", "EKF_AM_XCD", "EKF_CHAIN_FAST")
PIPE = {"EKF_RESIDENT": "0"}
FORMS = pytest.mark.parametrize("joseph", [False, True], ids=["simple", "joseph"])
F64, F32 = pyekf.EKF_F64, pyekf.EKF_F32


def _ids(cases):
    return ["-".join(f"g{v:g}" if isinstance(v, float) else str(v) for v in c) for c in cases]


def _with_gates(names, psets):
    return [(n, p, g) for n in names for p in psets if (n, p) not in pc.LEFT_OUT
            for g in (pc.GATES if n in pc.ASSOC else pc.GATES[:1])]


@pytest.fixture(scope="module", autouse=True)
def _record_errors():
    yield
    es.write_errors("params", ERRORS)


def _env(monkeypatch, env):
    for k in ENV_KEYS:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def _handle(e, pset, gate, dtype, joseph, path=None, F=1):
    """Created after the environment is set: the settings are read at ekf_create."""
    h = pyekf.EKF(e.n_landmarks, F, dtype, **pc.params(pset, gate))
    if path is not None:
        assert h.path == path
    assert h.set_joseph(joseph) == pyekf.EKF_OK
    return h


def _arrays(edges, sl=slice(None)):
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
    return tuple(np.ascontiguousarray(a[sl]) for a in (cnt, ids, act, rel, od))


def _gpu(arrs):
    import torch
    return [torch.from_numpy(a).cuda() for a in arrs]


def _feed(h, e, how, ref, first=0):
    """Messages first.. of `e` through one submission form → every posterior pose [T - first, 3]
    (read per message, or from the pose trace after a replay). Under association the decisions
    equal the oracle's: message by message (sensor), the last message's (the replays)."""
    T = e.n_messages
    if how == "sensor":
        poses = np.zeros((T - first, 3))
        for t in range(first, T):
            c = int(e.count[t])
            assert h.set_odom(e.odom[t]) == 0
            if e.assoc:
                rc, j, nw = h.sensor(e.rel[t, :c])
                assert rc == 0
                assert np.array_equal(j, ref["assoc_j"][t, :c]), (t, j, ref["assoc_j"][t, :c])
                assert np.array_equal(nw, ref["assoc_new"][t, :c]), t
                assert h.state(sigma=False)[2] == ref["counters"][t]
            else:
                assert h.fake_sensor(e.ids[t, :c], e.actions[t, :c], e.rel[t, :c]) == 0
            poses[t - first] = h.pose()
        return poses
    h.trace_enable(T)
    cnt, ids, act, rel, od = _arrays([e], slice(first, T))
    if how == "replay":
        h.replay(cnt, rel, od, ids=None if e.assoc else ids, actions=act, assoc=e.assoc)
    elif how == "device":  # ekf_replay_resident / ekf_replay_device / ekf_replay_device_assoc
        g = _gpu((cnt, rel, od, ids, act))
        h.replay_on_device(g[0], g[1], g[2], ids=None if e.assoc else g[3],
                           actions=None if e.assoc else g[4])
        h.sync()  # (the tensors may go)
    else:
        raise ValueError(how)
    if e.assoc:
        c = int(e.count[T - 1])
        j, nw = h.decisions(c)
        assert np.array_equal(j, ref["assoc_j"][T - 1, :c]), (j, ref["assoc_j"][T - 1, :c])
        assert np.array_equal(nw, ref["assoc_new"][T - 1, :c])
    poses = h.trace()[0]
    assert poses.shape == (T - first, 3)
    return poses


def _compare(key, h, ref, tol, poses=None, first=0, f=0):
    x, S, cnt = h.state(f)
    assert h.status(f) == 0
    assert np.all(np.isfinite(x)) and np.all(np.isfinite(S))
    err = {"pose": float(np.abs(x[:3] - ref["state"][:3]).max()),
           "state": float(np.abs(x - ref["state"]).max()),
           "sigma": float(np.abs(S - ref["sigma"]).max()),
           "tmo": float(np.abs(h.map_odom(f) - ref["tmo"]).max())}
    if poses is not None:
        err["pose"] = max(err["pose"], float(np.abs(poses - ref["poses"][first:]).max()))
    ERRORS[key] = err
    print(key, err)
    assert cnt == ref["counter"]
    assert err["pose"] < tol[0], err
    assert err["tmo"] < tol[1], err
    assert err["state"] < tol[1], err
    assert err["sigma"] < tol[2], err


def _tol(dtype, assoc):
    if dtype == F32:
        return es.F32_TOL
    return es.ASSOC_TOL if assoc else es.KNOWN_TOL


def _run(monkeypatch, key, env, name, pset, gate, dtype, joseph, how, path, warm=False,
         check=None):
    """One case: the environment, a handle at the set's parameters, (the warm start,) every
    message through `how`, the comparison with the oracle at the same parameters and form."""
    _env(monkeypatch, env)
    e = pc.get(name)
    ref = pc.oracle(name, pset, gate, joseph=joseph)
    h = _handle(e, pset, gate, dtype, joseph, path)
    first = 0
    if warm:
        x, S, tmo, cnt = pc.oracle_warm(name, pset, gate, joseph)
        h.set_state(x, S, tmo=tmo, counter=cnt)
        first = pc.WARM
    poses = _feed(h, e, how, ref, first)
    if check is not None:
        check(h)
    form = "joseph" if joseph else "simple"
    _compare(f"{key}/{name}/{pset}/g{gate:g}/{form}/{how}", h, ref, _tol(dtype, e.assoc), poses,
             first)
    h.close()


# ---- the resident path: k_resident per message and per replay, k_resident_replay -----------------
RESIDENT = _with_gates(("known20", "assoc20"), pc.SETS)


@FORMS
@pytest.mark.parametrize("how", ["sensor", "replay", "device"])
@pytest.mark.parametrize("name,pset,gate", RESIDENT, ids=_ids(RESIDENT))
def test_resident_against_oracle(monkeypatch, name, pset, gate, how, joseph):
    """predict (Q on the pose block), innovation_gain and score_and_decide (R), the prior of a
    landmark's first sighting: per-message calls, ekf_replay and ekf_replay_resident."""
    _run(monkeypatch, "resident", {}, name, pset, gate, F64, joseph, how,
         pyekf.EKF_PATH_RESIDENT)


# ---- the pipeline, default settings --------------------------------------------------------------
PIPELINE = _with_gates(pc.KNOWN + pc.ASSOC, pc.SETS)
# (ekf_replay_device takes one chunk per message: known24x20's 20 markers go through ekf_replay)
PIPE_HOW = [(n, p, g, how) for n, p, g in PIPELINE for how in ("replay", "device")
            if not (n == "known24x20" and how == "device")]


@FORMS
@pytest.mark.parametrize("name,pset,gate,how", PIPE_HOW, ids=_ids(PIPE_HOW))
def test_pipeline_fp64_against_oracle(monkeypatch, name, pset, gate, how, joseph):
    """k_factors' predicted pose block, the Σ pass and k_stage, the chain's fold, rebuild and
    wave-0 steps; k_assoc_msg's predict_pose_block, assoc_dist and pose_step with one workgroup
    (N = 20) and three (N = 130); planned on the host and on the device."""
    _run(monkeypatch, "pipe64", PIPE, name, pset, gate, F64, joseph, how,
         pyekf.EKF_PATH_PIPELINE)


@FORMS
@pytest.mark.parametrize("name,pset,gate", _with_gates(pc.ASSOC, pc.SETS),
                         ids=_ids(_with_gates(pc.ASSOC, pc.SETS)))
def test_pipeline_fp64_sensor_decisions(monkeypatch, name, pset, gate, joseph):
    """ekf_sensor with decision outputs on the pipeline: every message's decisions and counter."""
    _run(monkeypatch, "pipe64", PIPE, name, pset, gate, F64, joseph, "sensor",
         pyekf.EKF_PATH_PIPELINE)


# ---- the pipeline, one setting at a time ---------------------------------------------------------
def _two_sets(names, dtype=F64):
    """q_lt_r and tight_prior in fp64, low_prior (q_lt_r's noises) and tight_prior in fp32 — and
    on known130 in fp64 too (param_cases.LEFT_OUT)."""
    return [(n, "low_prior" if p == "q_lt_r" and (dtype == F32 or n == "known130") else p, g)
            for n, p, g in _with_gates(names, ("q_lt_r", "tight_prior"))
            ]


SETTINGS = ([("stage0", {"EKF_STAGE": "0"}, F64) + c for c in _two_sets(pc.KNOWN + pc.ASSOC)] +
            [("serial", {"EKF_SERIAL": "1"}, F64) + c for c in _two_sets(pc.KNOWN + pc.ASSOC)] +
            [("agent", {"EKF_AM_XCD": "0"}, F64) + c for c in _two_sets(pc.ASSOC)] +
            [("marker", {"EKF_ASSOC_MSG": "0"}, F64) + c for c in _two_sets(pc.ASSOC)] +
            [("marker", {"EKF_ASSOC_MSG": "0"}, F32) + c for c in _two_sets(pc.ASSOC, F32)])
SETTING_IDS = _ids([(c[0], "f64" if c[2] == F64 else "f32") + c[3:] for c in SETTINGS])


def _check_setting(what, name):
    def check(h):
        if what == "serial":
            assert h.schedule & pyekf.EKF_SCHED_SERIAL
        if what == "marker":
            assert h.assoc_route == pyekf.EKF_ASSOC_MARKER
        elif what == "agent" or name == "assoc20":
            assert h.assoc_route == pyekf.EKF_ASSOC_CHUNK
        elif name == "assoc130":
            assert h.assoc_route == pyekf.EKF_ASSOC_CHUNK_XCD
    return check


@FORMS
@pytest.mark.parametrize("what,env,dtype,name,pset,gate", SETTINGS, ids=SETTING_IDS)
def test_pipeline_settings_against_oracle(monkeypatch, what, env, dtype, name, pset, gate,
                                          joseph):
    """The chains gathering their own rebuild operands, one stream, the agent placement of
    k_assoc_msg's exchange, and one marker per launch (k_assoc; fp32 too, from the warm state).
    Under EKF_ASSOC_MSG=0 the replay is ekf_replay(assoc=1): the device-planned one needs
    k_assoc_msg."""
    _run(monkeypatch, f"{what}/{'f64' if dtype == F64 else 'f32'}", dict(PIPE, **env), name,
         pset, gate, dtype, joseph, "replay", pyekf.EKF_PATH_PIPELINE, warm=dtype == F32,
         check=_check_setting(what, name))


LEAN = [(d,) + c + (how,) for d in (F64, F32) for c in _two_sets(pc.KNOWN, d)
        for how in ("replay", "device") if not (c[0] == "known24x20" and how == "device")]
LEAN_IDS = _ids([("f64" if c[0] == F64 else "f32",) + c[1:] for c in LEAN])


@FORMS
@pytest.mark.parametrize("dtype,name,pset,gate,how", LEAN, ids=LEAN_IDS)
def test_lean_program_against_oracle(monkeypatch, dtype, name, pset, gate, how, joseph):
    """EKF_CHAIN_FAST=1: wave 0's lean program takes r through a lane-0 broadcast of its own.
    ekf_chain_path_counts shows that it ran: every correction of a message without a first
    sighting (a chunk goes to the generic program from its first one on; these drives hold no
    other event): all but message 0's on known20 and known24x20, 48 of 160 on known130."""
    e = pc.get(name)
    first = pc.WARM if dtype == F32 else 0
    seen, common = set(), 0
    for t in range(e.n_messages):
        now = set(e.ids[t, :int(e.count[t])].tolist())
        common += int(e.count[t]) if t >= first and now <= seen else 0
        seen |= now
    total = int(e.count[first:].sum())
    assert common >= 32

    def check(h):
        lean, generic = h.chain_path_counts()
        assert lean + generic == total and lean >= common, (lean, generic, total, common)

    _run(monkeypatch, f"lean/{'f64' if dtype == F64 else 'f32'}",
         dict(PIPE, EKF_CHAIN_FAST="1"), name, pset, gate, dtype, joseph, how,
         pyekf.EKF_PATH_PIPELINE, warm=dtype == F32, check=check)


# ---- the fp32 pipeline, default settings ---------------------------------------------------------
@FORMS
@pytest.mark.parametrize("name,pset,gate,how", PIPE_HOW, ids=_ids(PIPE_HOW))
def test_pipeline_fp32_from_warm_state(monkeypatch, name, pset, gate, how, joseph):
    """fp32 Σ from the fp64 state after param_cases.WARM messages. tight_prior under association
    drives pose_step's fp32 test "still at its prior" (kk >= 0.5 * prior) for landmarks that have
    been corrected (test_param_cases.py pins that): the chunk's block is patched for them and must
    still come out right."""
    _run(monkeypatch, "pipe32_warm", {}, name, pset, gate, F32, joseph, how,
         pyekf.EKF_PATH_PIPELINE, warm=True)


COLD = [c for c in PIPE_HOW if pc.SETS[c[1]][2] <= 1e3 and c[3] == "replay"]


@FORMS
@pytest.mark.parametrize("name,pset,gate,how", COLD, ids=_ids(COLD))
def test_pipeline_fp32_from_message_0(monkeypatch, name, pset, gate, how, joseph):
    """init_var <= 1e3: fp32 holds the prior's cancellation, so the whole run is in fp32."""
    _run(monkeypatch, "pipe32_cold", {}, name, pset, gate, F32, joseph, how,
         pyekf.EKF_PATH_PIPELINE)


@FORMS
@pytest.mark.parametrize("name,pset,gate", _with_gates(pc.ASSOC, ("low_prior", "tight_prior")),
                         ids=_ids(_with_gates(pc.ASSOC, ("low_prior", "tight_prior"))))
def test_pipeline_fp32_marker_route(monkeypatch, name, pset, gate, joseph):
    """fp32 under EKF_ASSOC_MSG=0 (k_assoc, one marker per launch), message by message with
    decisions, from the warm state."""
    _run(monkeypatch, "marker/f32_sensor", dict(PIPE, EKF_ASSOC_MSG="0"), name, pset, gate, F32,
         joseph, "sensor", pyekf.EKF_PATH_PIPELINE, warm=True,
         check=_check_setting("marker", name))


# ---- a swarm -------------------------------------------------------------------------------------
@FORMS
@pytest.mark.parametrize("path", ["resident", "pipe64"])
def test_swarm_of_three_against_their_oracles(monkeypatch, path, joseph):
    """n_filters = 3 at q_gt_r: known20, known20 with every message's markers in reverse order,
    known20 with no message on every second step. Each filter equals its own oracle run: the
    parameters reach every filter of the handle, and a filter that sits a step out takes no Q."""
    _env(monkeypatch, {} if path == "resident" else PIPE)
    base = pc.get("known20")
    edges = [base, pc.reversed_markers(base), pc.every_second_silent(base)]
    h = _handle(base, "q_gt_r", 2.0, F64, joseph,
                pyekf.EKF_PATH_RESIDENT if path == "resident" else pyekf.EKF_PATH_PIPELINE, F=3)
    cnt, ids, act, rel, od = _arrays(edges)
    h.replay(cnt, rel, od, ids=ids, actions=act)
    for f, e in enumerate(edges):
        _compare(f"swarm/{path}/{'joseph' if joseph else 'simple'}/{f}", h,
                 pc.run_swarm_oracle(e, "q_gt_r", joseph), es.KNOWN_TOL, f=f)
    h.close()


# ---- Σ₀: ekf_create and ekf_reset ----------------------------------------------------------------
@pytest.mark.parametrize("path", ["resident", "pipe64", "pipe32"])
@pytest.mark.parametrize("pset", list(pc.SETS))
def test_sigma0_is_the_configured_prior(monkeypatch, pset, path):
    """Right after ekf_create, and after a message and ekf_reset: ekf_get_state returns
    diag(0, 0, 0, init_var, ...) exactly and ekf_get_marginals every landmark's variance as
    init_var exactly, in both filters of the handle."""
    _env(monkeypatch, PIPE if path == "pipe64" else {})
    e = pc.get("known20")
    prior = pc.SETS[pset][2]
    h = _handle(e, pset, 2.0, F32 if path == "pipe32" else F64, False,
                pyekf.EKF_PATH_RESIDENT if path == "resident" else pyekf.EKF_PATH_PIPELINE, F=2)
    want = np.diag(np.r_[np.zeros(3), np.full(2 * e.n_landmarks, prior)])

    def check():
        for f in range(2):
            x, S, cnt = h.state(f)
            assert cnt == 0 and not x.any()
            np.testing.assert_array_equal(S, want)
            pose, cov, lm, cnt = h.marginals(f)
            assert cnt == 0 and not pose.any() and not cov.any() and not lm["seen"].any()
            np.testing.assert_array_equal(lm["cov"], np.tile([prior, 0.0, prior],
                                                             (e.n_landmarks, 1)))

    check()
    c = int(e.count[0])
    for f in range(2):
        assert h.set_odom(e.odom[0], f) == 0
        assert h.fake_sensor(e.ids[0, :c], e.actions[0, :c], e.rel[0, :c], f) == 0
    assert h.state()[1][3 + 2 * int(e.ids[0, 0]), 3 + 2 * int(e.ids[0, 0])] < prior
    h.reset()
    check()
    h.close()


# ---- slam_create takes the ekf_config ------------------------------------------------------------
@FORMS
def test_slam_node_takes_the_parameters(monkeypatch, joseph):
    """known20's wheel ticks and markers through slam_replay on a node created with q_lt_r,
    against orc.run_scenario at the same parameters: every pose, the state, Σ."""
    _env(monkeypatch, {})
    sc = pc.scenario("known20")
    par = pc.params("q_lt_r")
    s = pyekf.Slam(n_landmarks=sc.n_landmarks, source=pyekf.SOURCE_SIM, **par)
    assert s.set_joseph(joseph) == pyekf.EKF_OK
    rc, poses, tmo = s.replay(sc)
    x, S, cnt = s.filter_state()
    s.close()
    assert rc == pyekf.EKF_OK
    o = orc.run_scenario(sc, False, joseph=joseph, **par)
    err = {"pose": float(np.abs(poses - o["poses"]).max()),
           "tmo": float(np.abs(tmo - o["tmo"]).max()),
           "state": float(np.abs(x - o["state"]).max()),
           "sigma": float(np.abs(S - o["sigma"]).max())}
    ERRORS[f"slam/known20/q_lt_r/{'joseph' if joseph else 'simple'}"] = err
    assert cnt == o["counter"]
    assert err["pose"] < es.KNOWN_TOL[0] and err["tmo"] < es.KNOWN_TOL[1], err
    assert err["state"] < es.KNOWN_TOL[1] and err["sigma"] < es.KNOWN_TOL[2], err
