"""The filter's own parameters away from their defaults: parameter sets, scenarios, oracle runs.

ekf_config's q_noise and r_noise default to the same 1e-2 and init_var to 1e7, and every other
scenario of the suite runs at those values: a kernel that read r where it needs q, or kept a
literal 1e-2 or 1e7, would compute the same thing there. The sets here make q != r, neither 1e-2,
and move the landmark prior; both noises stay below 1e-2, so Σ's populated entries are no larger
than at the defaults and the suite's absolute bounds (edge_scenarios.KNOWN_TOL / ASSOC_TOL /
F32_TOL) carry over unscaled. Every init_var is exactly representable in fp32. No prior above 1e7:
at 1e9 the oracle's own two arithmetic modes differ by 1.5e-8 to 7e-6 on these scenarios.

tight_prior (init_var = 2^-8 < r) is built for k_assoc_msg's fp32 test "still at its prior"
(kk >= 0.5 * prior): a corrected landmark's variance stays near prior * r / (prior + r) = 2.6e-3,
above 0.5 * prior = 1.95e-3, so the test fires for landmarks that have been corrected and the
chunk's block is patched for them; the chunk must still come out right.

The scenarios are pyekf.synth drives that edge_scenarios already uses, as edge_scenarios.Edge
(odometry by the oracle's DiffDrive: the oracle and the GPU see the same bits). tests/
test_param_cases.py pins each (scenario, set, gate, form) with the oracle alone; tests/
test_gpu_params.py replays them through the product.
"""
from __future__ import annotations

import numpy as np

import edge_scenarios as es
from pyekf import synth

DEFAULT_Q = DEFAULT_R = 1e-2
DEFAULT_PRIOR = 10e6
# name → (q_noise, r_noise, init_var)
SETS = {
    "q_lt_r": (2.5e-3, 8e-3, DEFAULT_PRIOR),
    "q_gt_r": (8e-3, 2.5e-3, DEFAULT_PRIOR),
    "low_prior": (2.5e-3, 8e-3, 1e3),
    "low_prior_qr": (8e-3, 2.5e-3, 1e3),
    "tight_prior": (2.5e-3, 8e-3, 2.0 ** -8),
}
GATES = (2.0, 3.0)  # under association every set runs at both
KNOWN = ("known20", "known24x20", "known130")
ASSOC = ("assoc20", "assoc130")
# assoc130's drive is edge_scenarios.assoc_zero(130, ..)'s with another seed. With that one's seed
# 18 the oracle's two modes differ by 5.4e-9 in the state (q_lt_r, Joseph), over the tenth of
# ASSOC_TOL's 5e-8 that the conditioning pin allows. Of the seeds 12 and 19..25 (pose / state / Σ
# over the two 1e7-prior sets, both gates, both forms: 12 4.9e-10 / 1.6e-9 / 5.1e-9, 19 5.0e-10 /
# 1.3e-9 / 2.0e-9, 20 9.2e-10 / 5.2e-9 / 3.1e-9, 22 6.4e-10 / 2.5e-9 / 2.6e-9, 23 7.6e-10 /
# 3.8e-9 / 2.4e-9, 24 6.9e-10 / 4.9e-9 / 2.5e-9, 25 7.5e-10 / 2.9e-9 / 2.6e-9) 21 is the best
# conditioned: 2.4e-10 / 6.2e-10 / 2.2e-9.
ASSOC130_SEED = 21
# known130 with the 1e7 prior is left out. Its 16 nearest of 100 landmarks change as the robot
# moves, so first sightings go on to the last message, and each leaves 1e7 - (1e7 - d) in Σ, one
# ulp of 1e7 (1.9e-9) apart between two faithful evaluation orders: the oracle's two modes differ
# by 2.6e-9 to 3.9e-9 in Σ on every drive seed tried (18..25; 2.6e-9 on 18), over the tenth of
# KNOWN_TOL's 1e-8 that the conditioning pin allows, and no seed can change that. (On known20 and
# known24x20 every landmark is sighted in message 0 and corrected in every message after it, which
# shrinks that difference to 1e-10.) The three sets with a smaller prior, which hold both (q, r)
# pairs, condition to 3e-13 and run on it.
LEFT_OUT = {("known130", "q_lt_r"), ("known130", "q_gt_r")}


def scenario(name: str):
    """The synth.Scenario (wheel ticks and marker arrays) behind the named case."""
    if name == "known20":      # one chunk per message
        sc = synth.make_scenario(20, synth.random_landmarks(12, seed=7), 12, max_markers=12,
                                 seed=8)
    elif name == "known24x20":  # two chunks per message: the predict's Q enters on the first only
        sc = synth.make_scenario(24, synth.random_landmarks(20, seed=7), 12, max_markers=20,
                                 seed=8)
    elif name == "known130":   # n = 263: sigma_grid.hpp's region grid (from N = 111); pipeline only
        sc = synth.make_scenario(130, synth.random_landmarks(100, seed=11), 10, max_markers=16,
                                 seed=18)
    elif name == "assoc20":
        sc = synth.make_scenario(20, synth.random_landmarks(12, seed=7), 10, max_markers=16,
                                 seed=14, shuffle=True)
    elif name == "assoc130":   # three k_assoc_msg workgroups per filter
        sc = synth.make_scenario(130, synth.random_landmarks(100, seed=11), 10, max_markers=16,
                                 seed=ASSOC130_SEED, shuffle=True)
    else:
        raise ValueError(name)
    return sc


def _build(name: str) -> es.Edge:
    e = es._edge(name, scenario(name), assoc=name in ASSOC)
    if e.assoc:
        e.ids[:] = -1
    return e


_edges: dict = {}
_runs: dict = {}


def get(name: str) -> es.Edge:
    """The named scenario, built once per process (treat it as read-only)."""
    if name not in _edges:
        _edges[name] = _build(name)
    return _edges[name]


def params(pset: str, gate: float = 2.0) -> dict:
    """The set as ekf_config / OracleEKF keyword arguments."""
    q, r, prior = SETS[pset]
    return dict(q_noise=q, r_noise=r, init_var=prior, mah_gate=gate)


def oracle(name: str, pset, gate: float = 2.0, literal=False, joseph=False):
    """edge_scenarios.run_oracle of a scenario at a parameter set (a name of SETS, or a (q, r,
    init_var) tuple), once per process: poses, state, Σ, decisions, dmin (read-only)."""
    q, r, prior = SETS[pset] if isinstance(pset, str) else pset
    key = (name, q, r, prior, gate, literal, joseph)
    if key not in _runs:
        _runs[key] = es.run_oracle(get(name), literal=literal, joseph=joseph, q_noise=q,
                                   r_noise=r, init_var=prior, mah_gate=gate)
    return _runs[key]


WARM = 4  # messages of the fp64 warm start that the fp32 cases continue from


def oracle_warm(name: str, pset: str, gate: float = 2.0, joseph=False):
    """The structured oracle's (state, sigma, tmo, counter) after the first WARM messages: what an
    fp32 handle is loaded with (ekf_set_state) before it runs the rest. The oracle going on from
    there is the whole run of `oracle` (its prev is the posterior pose, as ekf_set_state's)."""
    import orc
    key = ("warm", name, pset, gate, joseph)
    if key not in _runs:
        e = get(name)
        ref = orc.OracleEKF(n_landmarks=e.n_landmarks, joseph=joseph, **params(pset, gate))
        for t in range(WARM):
            c = int(e.count[t])
            ref.set_odom(e.odom[t])
            rc = (ref.sensor_cb(e.rel[t, :c])[0] if e.assoc else
                  ref.fake_sensor_cb(e.ids[t, :c], e.actions[t, :c], e.rel[t, :c]))
            assert rc == 0
        _runs[key] = ref.get()
    return _runs[key]


def cases():
    """(scenario, set, gate) of every case: the known-id scenarios at the default gate (they never
    read it; without LEFT_OUT), the association ones at both."""
    return ([(n, p, GATES[0]) for n in KNOWN for p in SETS if (n, p) not in LEFT_OUT] +
            [(n, p, g) for n in ASSOC for p in SETS for g in GATES])


def reversed_markers(e: es.Edge) -> es.Edge:
    """`e` with each message's markers in reverse order (another filter of a swarm)."""
    ids, act, rel = e.ids.copy(), e.actions.copy(), e.rel.copy()
    for t in range(e.n_messages):
        c = int(e.count[t])
        ids[t, :c], act[t, :c], rel[t, :c] = e.ids[t, :c][::-1], e.actions[t, :c][::-1], \
            e.rel[t, :c][::-1]
    return es.Edge(e.name + "_rev", e.n_landmarks, e.count.copy(), ids, act, rel, e.odom.copy())


def every_second_silent(e: es.Edge) -> es.Edge:
    """`e` with no markers (count 0: no message for the filter) on messages 1, 3, 5, ..."""
    cnt = e.count.copy()
    cnt[1::2] = 0
    return es.Edge(e.name + "_half", e.n_landmarks, cnt, e.ids.copy(), e.actions.copy(),
                   e.rel.copy(), e.odom.copy())


def run_swarm_oracle(e: es.Edge, pset: str, joseph=False):
    """The oracle through a known-id Edge whose messages may be absent (count 0: neither the
    odometry nor a predict reaches the filter, as in a replay) → state, sigma, tmo, counter."""
    import orc
    ref = orc.OracleEKF(n_landmarks=e.n_landmarks, joseph=joseph, **params(pset))
    for t in range(e.n_messages):
        c = int(e.count[t])
        if c == 0:
            continue
        ref.set_odom(e.odom[t])
        assert ref.fake_sensor_cb(e.ids[t, :c], e.actions[t, :c], e.rel[t, :c]) == 0
    x, S, tmo, cnt = ref.get()
    return dict(state=x, sigma=S, tmo=tmo, counter=cnt)
