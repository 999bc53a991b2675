"""The host planner (ekf-slam_amd/csrc/ekf_plan.cpp) against recorded bytes, on the CPU alone.

tests/plan_host_main.cpp replays a fixed script of planner calls: known association at the chunk
edges (m = 0 with every marker a DELETE, 1, 16, 17, 33), three filters of unequal length with one
absent, runs of messages long enough for kStageOut two chunks back and kStageIn after it, staging
off, the resident path, the Joseph form and a switch of it, predict = false with a pending predict,
the posterior alone, unknown association on both routes (0, 1, 16, 17, 64, 65, 130 markers, one
window and windows of 64), rejected batches, a PlanState export → adopt round trip and what a
device-written plan leaves. It is compiled with the host compiler together with ekf_plan.cpp under
AddressSanitizer + UndefinedBehaviorSanitizer and run as a program of its own.

Per section of the script the MsgDesc bytes, the launch list (kind, off, f0, nf, kw, and the two
queries the scheduler asks: "some active filter has no kLook", "some active filter stages"), the
return codes of the message input and the final mirror (parity, pending, prev_m, prev_ids) must
equal tests/golden/plan/sections.bin.gz (the driver's output, gzipped). The fixture was recorded
from the runtime as it was before the planner was split out of it (the same script through an
adapter over that ekf_api.cpp's plan_known / plan_unknown / plan_posterior / load_batch), not from
the code under test."""
import gzip
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ekf-slam_amd", "csrc")
GOLDEN = os.path.join(ROOT, "tests", "golden", "plan", "sections.bin.gz")
DESC_BYTES = 576        # sizeof(MsgDesc)
MIRROR_INTS = 3 + 16    # parity, pending, prev_m, prev_ids[kMaxChunk]


def parse(buf):
    """The driver's output → {section: {desc, launch, rc, mirror}} in script order."""
    out, o = {}, 0
    while o < len(buf):
        name = buf[o:o + 48].split(b"\0")[0].decode()
        F, nd, nl, nrc = np.frombuffer(buf, np.int32, 4, o + 48)
        o += 64
        sec = {}
        for key, dt, cnt in (("desc", np.uint8, nd * DESC_BYTES), ("launch", np.int32, nl * 7),
                             ("rc", np.int32, nrc), ("mirror", np.int32, F * MIRROR_INTS)):
            sec[key] = np.frombuffer(buf, dt, cnt, o)
            o += sec[key].nbytes
        assert name not in out, name
        out[name] = sec
    assert o == len(buf)
    return out


@pytest.fixture(scope="module")
def sections(tmp_path_factory):
    cxx = shutil.which("c++") or shutil.which("g++")
    assert cxx, "no host C++ compiler"
    tmp = tmp_path_factory.mktemp("plan_host")
    exe, dst = str(tmp / "plan_host_main"), str(tmp / "sections.bin")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", os.path.join(ROOT, "include"), "-I", CSRC,
                    os.path.join(ROOT, "tests", "plan_host_main.cpp"),
                    os.path.join(CSRC, "ekf_plan.cpp"), "-o", exe], check=True)
    # the harness may preload a library of its own: ASan must not insist on coming first
    env = dict(os.environ, ASAN_OPTIONS="verify_asan_link_order=0:detect_leaks=1:abort_on_error=0",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([exe, dst], capture_output=True, text=True, env=env, timeout=120)
    assert r.returncode == 0, r.stderr[-4000:]
    assert "runtime error" not in r.stderr and "Sanitizer" not in r.stderr, r.stderr[-4000:]
    with open(dst, "rb") as fh:
        return parse(fh.read())


@pytest.fixture(scope="module")
def golden():
    with gzip.open(GOLDEN, "rb") as fh:
        return parse(fh.read())


def test_script_covers_the_recorded_sections(sections, golden):
    assert set(sections) == set(golden)
    # the script reaches what it is there for
    flags = np.concatenate([s["desc"].reshape(-1, DESC_BYTES)[:, 4:8].copy().view(np.int32).ravel()
                            for s in sections.values()])
    for bit in (1, 2, 4, 8, 16, 128, 256, 512):   # kFirst … kStageIn
        assert np.any(flags & bit), bit
    kinds = np.concatenate([s["launch"].reshape(-1, 7)[:, 0] for s in sections.values()])
    assert set(kinds.tolist()) == {0, 1, 2, 3}
    rcs = np.concatenate([s["rc"] for n, s in sections.items() if n != "plan_state.export"])
    assert {0, -1, -2} <= set(rcs.tolist())       # EKF_OK, EKF_E_ARG, EKF_E_RANGE


def test_planner_matches_recorded_bytes(sections, golden):
    bad = []
    for name, sec in sections.items():
        for part in ("desc", "launch", "rc", "mirror"):
            got, want = sec[part], golden[name][part]
            if got.shape != want.shape or not np.array_equal(got, want):
                if part == "desc" and got.shape == want.shape:
                    d = np.flatnonzero(got != want)[0]
                    bad.append(f"{name}/desc: descriptor {d // DESC_BYTES}, byte {d % DESC_BYTES}")
                else:
                    bad.append(f"{name}/{part}: {got.tolist()[:40]} != {want.tolist()[:40]}")
    assert not bad, "\n".join(bad[:20])
