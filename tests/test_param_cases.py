"""The parameter cases of tests/param_cases.py, pinned with the oracle alone (no GPU).

tests/test_gpu_params.py runs these cases through the product and compares with the structured
oracle at the same parameters. For that to mean something, every (scenario, set, gate, form) must

* be well conditioned: the oracle's literal dense arithmetic and its structured restatement agree
  ten times tighter than the fp64 bound the GPU test applies, take the same decisions, and keep
  every decision more than 1e-3 from the gate;
* run the common case only: every message returns 0;
* be able to see a wrong parameter: the oracle with q and r exchanged, and the oracle at the
  default q = r = 1e-2 (same init_var and gate), each land at least 1e-4 away in the final pose or
  in the state, four orders of magnitude above the fp64 bounds and twenty times the fp32 ones.

A case that fails a pin is re-seeded or dropped, never given a wider bound. The third restatement,
oracle/ekf_numpy.py, takes the parameters too and agrees with the C oracle.
"""
import numpy as np
import pytest

import edge_scenarios as es
import param_cases as pc

FORMS = pytest.mark.parametrize("joseph", [False, True], ids=["simple", "joseph"])
CASES = pytest.mark.parametrize("name,pset,gate", pc.cases(),
                                ids=[f"{n}-{p}-g{g:g}" for n, p, g in pc.cases()])
GATE_MARGIN = 1e-3
SENSITIVITY = 1e-4


def test_sets_are_what_they_claim():
    """q != r, neither the default, both below it; init_var exact in fp32; one prior below r."""
    for q, r, prior in pc.SETS.values():
        assert q != r and q < pc.DEFAULT_Q and r < pc.DEFAULT_R
        assert float(np.float32(prior)) == prior and prior <= pc.DEFAULT_PRIOR
    q, r, prior = pc.SETS["tight_prior"]
    assert prior < r and prior * r / (prior + r) >= 0.5 * prior
    assert {(q, r) for q, r, _ in pc.SETS.values()} == {(2.5e-3, 8e-3), (8e-3, 2.5e-3)}


def test_scenario_shapes():
    """One chunk per message, two chunks, the region grid's size, three association workgroups."""
    e = pc.get("known20")
    assert e.n_landmarks == 20 and e.count.max() <= 16 and e.n_messages == 12
    e = pc.get("known24x20")
    assert e.n_landmarks == 24 and e.count.min() == 20 and e.n_messages == 12
    e = pc.get("known130")
    assert e.n_landmarks == 130 and 3 + 2 * e.n_landmarks == 263 and e.count.max() <= 16
    for name in pc.ASSOC:
        e = pc.get(name)
        assert e.assoc and np.all(e.ids == -1) and e.count.max() <= 16 and e.n_messages == 10
    assert pc.get("assoc130").n_landmarks == 130 and pc.get("assoc20").n_landmarks == 20
    for name in pc.KNOWN + pc.ASSOC:
        assert pc.get(name).count.min() > 0
    # known20 / known24x20 sight every landmark in every message (first sightings in message 0
    # only); known130's nearest 16 change along the drive (param_cases.LEFT_OUT)
    for name in ("known20", "known24x20"):
        e = pc.get(name)
        assert all(set(e.ids[t]) == set(e.ids[0]) for t in range(e.n_messages))
    e = pc.get("known130")
    assert set(e.ids[-1]) - set(e.ids[:-1].ravel())
    assert all((n, p) in {(a, b) for a, b, _ in pc.cases()} or (n, p) in pc.LEFT_OUT
               for n in pc.KNOWN + pc.ASSOC for p in pc.SETS)
    assert all(pc.SETS[p][2] == pc.DEFAULT_PRIOR for _, p in pc.LEFT_OUT)


@FORMS
@CASES
def test_case_is_well_conditioned(name, pset, gate, joseph):
    """Measured worst cases with the 1e7 prior over both sets, gates and forms, pose / state / Σ
    between the two modes: known20 2.5e-10 / 6.1e-10 / 3.3e-10, known24x20 2.0e-10 / 4.2e-10 /
    2.2e-10, assoc20 3.4e-10 / 5.5e-10 / 3.1e-9, assoc130 (seed 21) 2.4e-10 / 6.3e-10 / 2.2e-9;
    every init_var <= 1e3 case under 4e-13. Smallest |dmin - gate|: 2.3e-2 (assoc20, low_prior,
    gate 2.0)."""
    e = pc.get(name)
    a = pc.oracle(name, pset, gate, False, joseph)
    b = pc.oracle(name, pset, gate, True, joseph)
    for o in (a, b):
        assert not o["rcs"].any(), o["rcs"]
        assert np.all(np.isfinite(o["state"])) and np.all(np.isfinite(o["sigma"]))
        assert np.all(np.isfinite(o["poses"]))
    assert np.array_equal(a["assoc_j"], b["assoc_j"])
    assert np.array_equal(a["assoc_new"], b["assoc_new"])
    assert a["counter"] == b["counter"]
    if e.assoc:
        assert a["counter"] > 0 and np.any((a["assoc_new"] == 0) & (a["assoc_j"] >= 0))
        for o in (a, b):
            d = o["dmin"][np.isfinite(o["dmin"])]
            assert d.size > 0 and np.abs(d - gate).min() > GATE_MARGIN
    pt, st, sg = es.ASSOC_TOL if e.assoc else es.KNOWN_TOL
    err = (np.abs(a["poses"] - b["poses"]).max(), np.abs(a["state"] - b["state"]).max(),
           np.abs(a["sigma"] - b["sigma"]).max())
    print(f"modes {name} {pset} {gate} {joseph}: {err[0]:.2e} {err[1]:.2e} {err[2]:.2e}")
    assert err[0] <= pt / 10, err
    assert err[1] <= st / 10, err
    assert err[2] <= sg / 10, err


@CASES
def test_forms_take_the_same_decisions(name, pset, gate):
    a, j = pc.oracle(name, pset, gate), pc.oracle(name, pset, gate, joseph=True)
    assert np.array_equal(a["assoc_j"], j["assoc_j"])
    assert np.array_equal(a["assoc_new"], j["assoc_new"])
    assert a["counter"] == j["counter"]


def _apart(a, b):
    """(final pose, state) distances of two oracle runs; under association a different landmark
    count is a difference no bound could miss."""
    if a["counter"] != b["counter"]:
        return np.inf, np.inf
    return (float(np.abs(a["poses"][-1] - b["poses"][-1]).max()),
            float(np.abs(a["state"] - b["state"]).max()))


@FORMS
@CASES
def test_case_sees_a_wrong_parameter(name, pset, gate, joseph):
    """The proof that the GPU comparison can detect a swapped or hard-coded noise parameter: the
    oracle at (r, q) and at the default (1e-2, 1e-2), init_var and gate kept, differs from the
    case's own run by at least 1e-4 in the final pose or in the state. Measured: 1.03e-4 at the
    least (known20, tight_prior, against the defaults), 1e-3 or more in most cases; under
    association some cases end with another landmark count."""
    q, r, prior = pc.SETS[pset]
    own = pc.oracle(name, pset, gate, joseph=joseph)
    for what, other in (("swapped", (r, q, prior)),
                        ("default", (pc.DEFAULT_Q, pc.DEFAULT_R, prior))):
        dp, ds = _apart(own, pc.oracle(name, other, gate, joseph=joseph))
        print(f"apart {name} {pset} {gate} {joseph} {what}: pose {dp:.2e} state {ds:.2e}")
        assert dp >= SENSITIVITY or ds >= SENSITIVITY, (what, dp, ds)


@CASES
def test_case_sees_a_wrong_prior(name, pset, gate):
    """... and a hard-coded 1e7 where the set's prior is another. Every scenario leaves landmark
    slots unsighted, whose variances in the oracle's Σ are init_var exactly: the Σ comparison sees
    a wrong prior there whatever it does to the estimate. With tight_prior the estimate shows it
    too, by 1e-4 or more. (A prior of 1e3 is as uninformative as one of 1e7: the poses and the
    state move by 1e-7 between them, which the fp64 bounds see and the fp32 ones do not.)"""
    q, r, prior = pc.SETS[pset]
    own = pc.oracle(name, pset, gate)
    d = np.diag(own["sigma"])[3:].reshape(-1, 2)
    unseen = np.all(own["state"][3:].reshape(-1, 2) == 0.0, axis=1)
    assert unseen.any() and np.all(d[unseen] == prior) and np.all(d[~unseen] < prior)
    if pset == "tight_prior":
        dp, ds = _apart(own, pc.oracle(name, (q, r, pc.DEFAULT_PRIOR), gate))
        print(f"apart {name} {pset} {gate} prior: pose {dp:.2e} state {ds:.2e}")
        assert dp >= SENSITIVITY or ds >= SENSITIVITY, (dp, ds)


def test_tight_prior_keeps_corrected_landmarks_above_half_the_prior():
    """What tight_prior is for: after the drive every mapped landmark's variances are still at or
    above 0.5 * init_var, so k_assoc_msg's fp32 test (kk >= 0.5 * prior) fires for landmarks that
    have been corrected many times; with the 1e3 prior none is."""
    for name in pc.ASSOC:
        for pset, want in (("tight_prior", True), ("low_prior", False)):
            o = pc.oracle(name, pset, 2.0)
            prior = pc.SETS[pset][2]
            d = np.diag(o["sigma"])[3:3 + 2 * int(o["counter"])].reshape(-1, 2)
            above = np.any(d >= 0.5 * prior, axis=1)
            assert d.shape[0] > 0
            assert above.any() if want else not above.any(), (name, pset, d.max(), d.min())


@pytest.mark.parametrize("joseph", [False, True], ids=["simple", "joseph"])
@pytest.mark.parametrize("pset", ["q_lt_r", "tight_prior"])
@pytest.mark.parametrize("name", ["known20", "assoc20"])
def test_numpy_restatement_takes_the_parameters(name, pset, joseph):
    """oracle/ekf_numpy.DenseEKF at the same parameters against the C oracle, message by message,
    within test_oracle_golden.py's bounds between the two (state 1e-8, Σ 1e-7), decisions equal."""
    import ekf_numpy
    e = pc.get(name)
    q, r, prior = pc.SETS[pset]
    o = pc.oracle(name, pset, 2.0, joseph=joseph)
    d = ekf_numpy.DenseEKF(n_landmarks=e.n_landmarks, q_noise=q, r_noise=r, init_var=prior,
                           mah_threshold=2.0, joseph=joseph)
    for t in range(e.n_messages):
        c = int(e.count[t])
        d.t_odom_robot = tuple(e.odom[t])
        if e.assoc:
            dec = d.sensor_cb(e.rel[t, :c])
            assert [k for k, _ in dec] == o["assoc_j"][t, :c].tolist(), t
            assert [int(n) for _, n in dec] == o["assoc_new"][t, :c].tolist(), t
        else:
            d.fake_sensor_cb(e.ids[t, :c], e.actions[t, :c], e.rel[t, :c])
        assert np.abs(d.state[:3] - o["poses"][t]).max() < 1e-8, t
    assert d.counter == o["counter"] or not e.assoc
    assert np.abs(d.state - o["state"]).max() < 1e-8
    assert np.abs(d.sigma - o["sigma"]).max() < 1e-7
