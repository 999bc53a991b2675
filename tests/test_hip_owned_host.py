"""The handles' owning buffers (ekf-slam_amd/csrc/hip_owned.hpp) on the CPU alone.

A test cannot make hipMalloc fail, so the failure paths of the grow-only buffers are run here:
tests/hip_owned_host_main.cpp includes only the generic part of the header (HIP_OWNED_NO_HIP: no
HIP header, no HIP runtime) and instantiates it with a counting allocator that fails on request,
once without flags (DeviceBuf's manner) and once with flags (PinnedBuf's). It is compiled with the
host compiler under AddressSanitizer + UndefinedBehaviorSanitizer and run as a program of its own.

It asserts: reserve within capacity allocates nothing and keeps the pointer; growth frees the old
block exactly once and allocates one block of max(n, at_least); a failed allocation leaves the
buffer empty (null, capacity 0) with EKF_E_NOMEM and the allocator's "clear last error" hook
called, and a following reserve of a size that fitted before allocates again; all-or-nothing groups
(ensure_plan_state, ensure_am, the ring, the simulator's reserve) report failure for every failing
member and come back whole on a healthy retry; moves transfer ownership and empty the source; at
exit nothing is live and nothing was freed twice."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ekf-slam_amd", "csrc")


def test_owned_buffers_on_the_host(tmp_path):
    cxx = shutil.which("c++") or shutil.which("g++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "hip_owned_host_main")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", os.path.join(ROOT, "include"), "-I", CSRC,
                    os.path.join(ROOT, "tests", "hip_owned_host_main.cpp"), "-o", exe], check=True)
    # the harness may preload a library of its own: ASan must not insist on coming first
    env = dict(os.environ, ASAN_OPTIONS="verify_asan_link_order=0:detect_leaks=1:abort_on_error=0",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=120)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    assert "runtime error" not in r.stderr and "Sanitizer" not in r.stderr, r.stderr[-4000:]
    assert "device-style" in r.stdout and "pinned-style" in r.stdout, r.stdout


def test_generic_part_needs_no_hip():
    """The driver sees no HIP header: the default policies sit behind HIP_OWNED_NO_HIP."""
    with open(os.path.join(CSRC, "hip_owned.hpp")) as fh:
        head, _, tail = fh.read().partition("#ifndef HIP_OWNED_NO_HIP")
    assert tail and "hip/" not in head and "hipSuccess" not in head
    with open(os.path.join(ROOT, "tests", "hip_owned_host_main.cpp")) as fh:
        src = fh.read()
    assert "#define HIP_OWNED_NO_HIP" in src and "<hip/" not in src
