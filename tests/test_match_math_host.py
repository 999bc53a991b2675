"""The matching arithmetic of ekf_eval_match (ekf-slam_amd/csrc/match_math.hpp) against numpy, on
the CPU.

match_math.hpp is a host + device header: k_eval_match (ekf_eval.hip) calls it per truth landmark
and per slot. tests/match_math_host_main.cpp drives the same functions phase by phase (stage, scan
and claim, count) from a case file this test writes and writes the results back; the program is
compiled by the host compiler with -ffp-contract=off (as the kernel is) under AddressSanitizer +
UndefinedBehaviorSanitizer and run as a program of its own.

Everything is compared exactly: tests/match_ref.py restates the arithmetic operation for operation
(dx*dx + dy*dy, every product and the sum rounded on its own), so the squared distances have the
same bits, and the rest is comparisons and integers."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from match_ref import match_np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ekf-slam_amd", "csrc")
FIELDS = ("n_truth", "n_matched", "n_primary", "n_dup", "n_spurious", "n_missed")


def build_cases():
    rng = np.random.default_rng(20241020)
    c = {}
    # ties: slot 0 sits between two mirror images (truth 1 and 3), slot 1 on two equal copies
    # (truth 0 and 2): the lower k wins each time
    c["ties"] = (np.array([[1.0, 2.0], [-3.0, 0.5]]),
                 np.array([[-3.0, 0.75], [1.5, 2.0], [-3.0, 0.75], [0.5, 2.0], [9.0, 9.0]]), 1.0)
    # a NaN truth never wins, though it is the closest in its other coordinate and comes first
    c["nan"] = (np.array([[1.0, 1.0], [2.0, 2.0]]),
                np.array([[np.nan, 1.0], [1.0, np.nan], [np.nan, np.nan], [1.25, 1.0], [2.0, 2.5]]),
                1.0)
    # the gate: |(3, 4) - (0, 0)| = 5 exactly (25 = 5 * 5); slot 1 sits on its truth (distance 0)
    x = np.array([[3.0, 4.0], [7.0, -2.0], [20.0, 20.0]])
    t = np.array([[0.0, 0.0], [7.0, -2.0]])
    c["gate0"] = (x, t, 0.0)
    c["gate_exact"] = (x, t, 5.0)
    c["gate_below"] = (x, t, float(np.nextafter(5.0, 0.0)))
    c["gate_inf"] = (x, t, np.inf)
    # nothing to match
    c["all_nan"] = (x, np.full((4, 2), np.nan), np.inf)
    # claim by the lowest slot: slots 4, 1 and 6 at truth 0, slots 2 and 5 at truth 2, slot 3
    # unseen though it lies on a truth landmark's mirror, slot 0 spurious
    c["claim"] = (np.array([[50.0, 50.0], [1.01, 1.0], [-2.0, 3.02], [0.0, 0.0], [1.0, 1.02],
                            [-2.01, 3.0], [0.99, 1.0]]),
                  np.array([[1.0, 1.0], [0.0, 0.01], [-2.0, 3.0], [8.0, -8.0]]), 0.1)
    for i, (N, n_map) in enumerate([(1, 1), (9, 4), (40, 70), (70, 40), (64, 1024)]):
        t = rng.uniform(-5, 5, (n_map, 2))
        t[rng.random(n_map) < 0.2, rng.integers(0, 2)] = np.nan
        pick = rng.integers(0, n_map, N)
        x = np.where(np.isnan(t[pick]), 1.0, t[pick]) + rng.normal(size=(N, 2)) * 0.05
        x[rng.random(N) < 0.15] = 0.0
        x[rng.random(N) < 0.1] += 3.0
        c[f"random{i}"] = (x, t, 0.12)
    return c


@pytest.fixture(scope="module")
def run(tmp_path_factory):
    cxx = shutil.which("c++") or shutil.which("g++")
    assert cxx, "no host C++ compiler"
    d = tmp_path_factory.mktemp("match_math_host")
    exe = str(d / "match_math_host_main")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-ffp-contract=off",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", os.path.join(ROOT, "include"), "-I", CSRC,
                    os.path.join(ROOT, "tests", "match_math_host_main.cpp"), "-o", exe], check=True)
    cases = build_cases()
    data = [float(len(cases))]
    for x, t, md in cases.values():
        data += [float(len(x)), float(len(t)), md] + list(x.reshape(-1)) + list(t.reshape(-1))
    src, dst = str(d / "cases.bin"), str(d / "results.bin")
    np.array(data, np.float64).tofile(src)
    # a library preloaded into every process must not make ASan refuse to start
    env = dict(os.environ, ASAN_OPTIONS="verify_asan_link_order=0:detect_leaks=1:abort_on_error=0",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([exe, src, dst], capture_output=True, text=True, env=env, timeout=120)
    assert "runtime error" not in r.stderr and "Sanitizer" not in r.stderr, r.stderr[-4000:]
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stdout + r.stderr[-2000:]
    flat = np.fromfile(dst, np.float64)
    res, at = {}, 0
    for name, (x, t, md) in cases.items():
        N = len(x)
        res[name] = (flat[at:at + N].astype(np.int32), flat[at + N:at + 2 * N],
                     flat[at + 2 * N:at + 2 * N + 8])
        at += 2 * N + 8
    assert at == flat.size
    return cases, res


def check(cases, res, name):
    x, t, md = cases[name]
    match, rec, best, _ = match_np(x, t, md)
    got_match, got_best, got = res[name]
    assert (got_match == match).all(), (name, got_match, match)
    assert got_best.tobytes() == best.tobytes(), name     # the same bits, +inf where none
    for i, k in enumerate(FIELDS):
        assert got[i] == rec[k], (name, k, got[i], rec[k])
    assert got[6] == rec["max_match_dist"], name
    n_seen = int((~((x[:, 0] == 0) & (x[:, 1] == 0))).sum())
    assert got[7] == n_seen
    # the identities
    assert got[3] == got[1] - got[2] and got[5] == got[0] - got[2] and got[4] == n_seen - got[1]
    return got_match, got


def test_ties_go_to_the_lower_index(run):
    match, got = check(*run, "ties")
    assert list(match) == [1, 0]


def test_a_nan_truth_never_wins(run):
    match, got = check(*run, "nan")
    assert list(match) == [3, 4] and got[0] == 2          # two truth landmarks are there


def test_the_gate(run):
    m0, g0 = check(*run, "gate0")
    assert list(m0) == [-1, 1, -1] and g0[6] == 0.0       # distance 0 passes max_dist = 0
    me, ge = check(*run, "gate_exact")
    assert list(me) == [0, 1, -1] and ge[6] == 5.0        # <=: the exact distance passes
    mb, _ = check(*run, "gate_below")
    assert list(mb) == [-1, 1, -1]
    mi, gi = check(*run, "gate_inf")
    assert list(mi) == [0, 1, 1] and gi[4] == 0           # +inf: nothing seen is spurious


def test_all_nan_truth_matches_nothing(run):
    match, got = check(*run, "all_nan")
    assert (match == -1).all()
    assert tuple(got[:7]) == (0, 0, 0, 0, 3, 0, 0.0)
    assert np.isinf(run[1]["all_nan"][1]).all()


def test_claim_by_the_lowest_slot(run):
    match, got = check(*run, "claim")
    assert list(match) == [-1, 0, 2, -1, 0, 2, 0]
    # truth 0 belongs to slot 1, truth 2 to slot 2; slots 4, 5 and 6 are duplicates; truth 1 and 3
    # are missed; slot 0 is spurious, slot 3 unseen
    assert tuple(got[:6]) == (4, 5, 2, 3, 1, 2)


@pytest.mark.parametrize("i", range(5))
def test_random_cases(run, i):
    match, got = check(*run, f"random{i}")
    if i >= 2:
        assert got[1] > 0 and got[4] > 0
