"""The device planner of unknown-association replays against the host planner, on the CPU alone.

k_plan_assoc (ekf-slam_amd/csrc/plan_kernels.hip) takes every scalar field of a chunk descriptor
from plan_assoc (plan_assoc.hpp), a host + device function. tests/plan_assoc_host_main.cpp assembles
descriptors from it the way the kernel's lanes do and holds them against Planner::unknown's
(ekf_plan.cpp, route EKF_ASSOC_CHUNK, predict = posterior = true, one call per message, absent for
a count <= 0) byte for byte, z included, and the mirror it leaves against Planner::export_state's:
F = 3, T = 70, counts drawn from {-1, 0, 1, 15, 16, 17, 32, 33, 64, 70}, m_max in {16, 17, 64},
both forms, a starting mirror with parity 1 and a pending predict; plus three messages of counts
<= 0 only, after which the mirror must be the one it started with. The program is compiled with
the host compiler under AddressSanitizer + UndefinedBehaviorSanitizer, linked with ekf_plan.cpp and
run as a program of its own.

The second test: libekfslam.so exports the entry points of the device-planned association replay
and the headers declare them."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ekf-slam_amd", "csrc")
NEW = {"ekf.h": ("ekf_replay_device_assoc", "ekf_get_decisions"),
       "landmarks.h": ("lm_detect_device", "lm_fetch_markers", "lm_replay_into")}


@pytest.fixture(scope="module")
def report(tmp_path_factory):
    cxx = shutil.which("c++") or shutil.which("g++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path_factory.mktemp("plan_assoc_host") / "plan_assoc_host_main")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", os.path.join(ROOT, "include"), "-I", CSRC,
                    os.path.join(ROOT, "tests", "plan_assoc_host_main.cpp"),
                    os.path.join(CSRC, "ekf_plan.cpp"), "-o", exe], check=True)
    # a library preloaded into every process must not make ASan refuse to start
    env = dict(os.environ, ASAN_OPTIONS="verify_asan_link_order=0:detect_leaks=1:abort_on_error=0",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=120)
    assert "runtime error" not in r.stderr and "Sanitizer" not in r.stderr, r.stderr[-4000:]
    return r


def test_device_descriptors_equal_host_planner(report):
    assert report.returncode == 0, report.stdout[-4000:] + report.stderr[-2000:]
    assert report.stdout.strip().endswith("ok")


def test_script_reaches_what_it_is_there_for(report):
    cases = re.findall(r"case m_max (\d+) joseph (\d) T (\d+) idle (\d): compared (\d+) "
                       r"active (\d+) flags (\d+)", report.stdout)
    assert len(cases) == 12
    seen = set()
    for m_max, jos, T, idle, compared, active, flags in map(lambda c: tuple(map(int, c)), cases):
        C = (m_max + 15) // 16
        assert compared == T * C * 3
        seen.add((m_max, jos, idle))
        if idle:
            assert T == 3 and active == 0 and flags == 0
            continue
        assert T == 70                      # the parity scan's second round of 64 messages
        assert 0 < active < compared        # active and inactive chunks both
        want = 1 | 2 | 4 | 8 | (128 if jos else 0)   # kFirst, kLast, kNoInit, kActive, kJoseph
        assert flags == want
    assert seen == {(m, j, i) for m in (16, 17, 64) for j in (0, 1) for i in (0, 1)}


def test_device_bearing_is_libms_but_for_a_rare_last_bit(report):
    """atan2_rounded (atan2_dd.hpp), the bearing the device planner computes, against the host
    libm's atan2 on 20 000 points: never more than one ulp apart, equal on at least 99.5 %."""
    m = re.search(r"bearings (\d+) equal (\d+) beyond-1ulp (\d+)", report.stdout)
    assert m, report.stdout[-2000:]
    n, equal, far = map(int, m.groups())
    assert n == 20000 and far == 0 and equal >= n - n // 200, (n, equal, far)


def test_new_entry_points_exported_and_declared():
    import pyekf
    L = pyekf.lib()
    for header, names in NEW.items():
        src = open(os.path.join(ROOT, "include", header)).read()
        src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
        for name in names:
            assert re.search(r"\bint\s+%s\s*\(" % name, src), (header, name)
            assert hasattr(L, name), name
            assert name in pyekf.EXPORTS
