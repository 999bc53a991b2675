"""The C ABI of the lidar Monte-Carlo run (include/ekf_sim.h ekf_sim_lidar_config,
ekf_sim_lidar_config_default, ekf_sim_run_lidar; include/landmarks.h lm_fetch_ranges): declared,
exported, bound, the configuration's layout against the C compiler's, its defaults, and NULL handles
rejected — no GPU needed."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import pyekf
from pyekf.landmarks import Detector

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, "include")
ENTRY = {"ekf_sim_lidar_config_default": ("ekf_sim.h", "void"),
         "ekf_sim_run_lidar": ("ekf_sim.h", "int"),
         "lm_fetch_ranges": ("landmarks.h", "int")}
FIELDS = ("n_beams", "max_markers", "threshold", "obstacle_radius", "scan")

LAYOUT_C = r"""
#include <stddef.h>
#include <stdio.h>
#include "ekf_sim.h"
int main(void) {
  printf("%zu %zu", sizeof(ekf_sim_lidar_config), sizeof(lm_scan_config));
  printf(" %zu %zu %zu %zu %zu\n", offsetof(ekf_sim_lidar_config, n_beams),
         offsetof(ekf_sim_lidar_config, max_markers), offsetof(ekf_sim_lidar_config, threshold),
         offsetof(ekf_sim_lidar_config, obstacle_radius), offsetof(ekf_sim_lidar_config, scan));
  return 0;
}
"""


def header(name):
    src = open(os.path.join(INCLUDE, name)).read()
    return re.sub(r"/\*.*?\*/", "", src, flags=re.S)


def test_entry_points_declared_exported_and_bound():
    L = pyekf.lib()
    for name, (h, ret) in ENTRY.items():
        assert re.search(r"^%s\s+%s\s*\(" % (ret, name), header(h), flags=re.M), (name, h)
        assert hasattr(L, name), name
        assert name in pyekf.EXPORTS and name in pyekf.LATER_EXPORTS, name
        assert getattr(L, name).argtypes is not None, name
    assert callable(pyekf.Sim.run_lidar) and callable(Detector.fetch_ranges)
    assert issubclass(pyekf.LidarConfig, C.Structure)
    # the simulator's header brings the front-end's types with it
    assert re.search(r'#include\s+"landmarks.h"', header("ekf_sim.h"))
    assert re.search(r"typedef struct \{\s*int n_beams;\s*int max_markers;\s*double threshold;\s*"
                     r"double obstacle_radius;\s*lm_scan_config scan;\s*\} ekf_sim_lidar_config;",
                     header("ekf_sim.h"))


def test_config_layout_is_the_c_compilers(tmp_path):
    R = pyekf.LidarConfig
    assert tuple(n for n, _ in R._fields_) == FIELDS
    # by hand: two ints, two doubles, then lm_scan_config (7 eight-byte fields)
    assert C.sizeof(pyekf.ScanConfig) == 56
    assert C.sizeof(R) == 24 + 56
    assert [getattr(R, n).offset for n in FIELDS] == [0, 4, 8, 16, 24]
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    if cc is None:
        pytest.fail("no C compiler to take sizeof(ekf_sim_lidar_config) with")
    src = tmp_path / "layout.c"
    src.write_text(LAYOUT_C)
    exe = tmp_path / "layout"
    subprocess.run([cc, "-std=c99", "-Wall", "-Werror", "-I", INCLUDE, str(src), "-o", str(exe)],
                   check=True)
    got = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True,
                                          text=True).stdout.split()]
    assert got == [C.sizeof(R), C.sizeof(pyekf.ScanConfig)] + [getattr(R, n).offset for n in FIELDS]


def test_defaults():
    L = pyekf.lib()
    c = pyekf.LidarConfig()
    C.memset(C.byref(c), 0xFF, C.sizeof(c))
    L.ekf_sim_lidar_config_default(C.byref(c))
    assert (c.n_beams, c.max_markers, c.threshold, c.obstacle_radius) == (360, 32, 0.2, 0.038)
    k = pyekf.ScanConfig()
    L.lm_scan_config_default(C.byref(k))
    assert bytes(c.scan) == bytes(k)
    assert (c.scan.seed, c.scan.scan0, c.scan.arena_w, c.scan.arena_h, c.scan.range_min,
            c.scan.range_max, c.scan.sigma) == (20240317, 0, 10.0, 5.0, 0.11, 10.0, 0.0)
    L.ekf_sim_lidar_config_default(None)                       # a NULL is left alone
    # the binding's constructor: own fields, the scan's fields, the arena pair
    c = pyekf.lidar_config(n_beams=300, sigma=1e-3, range_max=3.5, arena=(40.0, 30.0), seed=9)
    assert (c.n_beams, c.max_markers, c.scan.sigma, c.scan.range_max, c.scan.arena_w,
            c.scan.arena_h, c.scan.seed) == (300, 32, 1e-3, 3.5, 40.0, 30.0, 9)
    with pytest.raises(TypeError):
        pyekf.lidar_config(beams=300)
    with pytest.raises(TypeError):
        pyekf.lidar_config(scan=k)


def test_null_handles_are_rejected_and_nothing_is_written():
    L = pyekf.lib()
    c = pyekf.lidar_config()
    cmd = np.zeros((40, 2))
    assert L.ekf_sim_run_lidar(None, None, 1, cmd.ctypes.data, C.byref(c)) == pyekf.EKF_E_ARG
    assert L.ekf_sim_run_lidar(None, None, 0, None, C.byref(c)) == pyekf.EKF_E_ARG
    out = np.full(4, 7.0, np.float32)
    assert L.lm_fetch_ranges(None, out.ctypes.data) == pyekf.EKF_E_ARG
    assert (out == 7.0).all()
