"""The Σ pass's tile grid (ekf-slam_amd/csrc/sigma_grid.hpp) on the CPU alone.

launch_sigma_pass sizes its grid from sigma_grid() and every wave of k_sigma_pass takes its
(filter, tile row, tile column) from sigma_grid_tile(): one definition, host + device.
tests/sigma_grid_host_main.cpp walks every (blockIdx.x, blockIdx.y, wave) of every grid through the
mapping and requires exactly the pass's tiles, each once (all of them for the full fp32 pass, the
ones with an element on or above the diagonal for the symmetric fp64 pass, worked out in the test),
no filter out of range, and the grid dimensions the launcher computed before the header existed:
tile shapes 32 x 32 full, 32 x 32 symmetric (< 16 filters) and 32 x 64 symmetric (>= 16 filters),
n = 1 ... 300, 513, 1025, 2051, with 1, 2, 15, 16, 17 and 24 filters. The program is compiled with
the host compiler under AddressSanitizer + UndefinedBehaviorSanitizer and run as a program of its
own."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ekf-slam_amd", "csrc")
SIZES = 303          # n = 1 ... 300, 513, 1025, 2051
FILTERS = (3, 3)     # filter counts below 16, from 16 on


@pytest.fixture(scope="module")
def report(tmp_path_factory):
    cxx = shutil.which("c++") or shutil.which("g++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path_factory.mktemp("sigma_grid_host") / "sigma_grid_host_main")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", CSRC,
                    os.path.join(ROOT, "tests", "sigma_grid_host_main.cpp"), "-o", exe], check=True)
    # a library preloaded into every process must not make ASan refuse to start
    env = dict(os.environ, ASAN_OPTIONS="verify_asan_link_order=0:detect_leaks=1:abort_on_error=0",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=120)
    assert "runtime error" not in r.stderr and "Sanitizer" not in r.stderr, r.stderr[-4000:]
    return r


def test_every_grid_covers_its_tiles_exactly_once(report):
    assert report.returncode == 0, report.stdout[-4000:] + report.stderr[-2000:]
    assert report.stdout.strip().endswith("ok")


def test_all_three_modes_reached_full_and_symmetric(report):
    modes = {m: (int(a), int(b)) for m, a, b in
             re.findall(r"mode (\w+): full (\d+) symmetric (\d+)", report.stdout)}
    assert set(modes) == {"plain", "xcd", "regions"}, report.stdout[-2000:]
    for m, (full, sym) in modes.items():
        assert full > 0 and sym > 0, modes
    few, many = FILTERS
    assert modes["xcd"] == (SIZES * many, SIZES * many)
    assert modes["plain"][0] + modes["regions"][0] == SIZES * few
    assert modes["plain"][1] + modes["regions"][1] == SIZES * few
