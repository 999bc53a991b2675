"""The simulated laser on the GPU (lm_simulate, ekf-slam_amd/csrc/lidar_kernels.hip) against its host
restatement synth.lidar_scans_counter, and its resident hand-off to the landmark front-end
(lm_detect_resident) against lm_detect and the oracles.

Range parity: every compared beam within one float32 step (np.spacing) of the restatement. Away
from grazing the two fp64 results differ by ≲ 2·10⁻¹⁰ m (cos / sin / sqrt / log to an ulp or two on
either side, magnified by ranges ≤ 10 m and at most 1024 minima), far below half a float32 step at
≥ 0.11 m (3.7·10⁻⁹), so the two roundings are equal or adjacent. A beam is left out only where the
restatement's |disc| < 1e-9 m² for some cylinder (a grazing ray, where hit and miss can flip), and
at most 0.5 % of a case's beams may be."""
import ctypes as C
import functools
import math

import numpy as np
import pytest

import landmarks_numpy as L
import orc
from test_gpu_pipeline import BASIC, _drive

pytestmark = pytest.mark.gpu

MAX_SCANS, MAX_BEAMS = 65, 2048
INC360 = float(np.float32(2 * math.pi / 360))


@pytest.fixture(scope="module")
def det():
    from pyekf.landmarks import Detector
    d = Detector(max_scans=MAX_SCANS, max_beams=MAX_BEAMS)
    yield d
    d.close()


def _dense():
    """1024 cylinders, r ∈ [0.03, 0.12], uniform in a 30 × 30 arena, none within 0.5 m of the
    origin; 3 poses near the origin."""
    rng = np.random.default_rng(7)
    out = []
    while len(out) < 1024:
        x, y = rng.uniform(-15.0, 15.0, 2)
        r = rng.uniform(0.03, 0.12)
        if math.hypot(x, y) - r >= 0.5:
            out.append((x, y, r))
    poses = np.array([(0.0, 0.0, 0.0), (1.0, 0.1, -0.05), (2.5, -0.08, 0.12)])
    return poses, np.array(out)


def _world():
    from pyekf import synth
    sc, obs, _ = synth.lidar_world(n_scans=40)
    return sc.truth, np.array(obs)


def _per_scan_scenes(S):
    rng = np.random.default_rng(S)
    scenes = np.asarray(BASIC)[None] + np.concatenate(
        [rng.uniform(-0.05, 0.05, (S, 1, 2)), np.zeros((S, 1, 1))], axis=2)
    return scenes, rng.permutation(S).astype(np.int32)


@functools.lru_cache(maxsize=None)
def _cases():
    dp, dc = _dense()
    c = {"drive40": dict(poses=_drive(40), circles=np.array(BASIC))}
    wp, wc = _world()
    c["lidar_world40"] = dict(poses=wp, circles=wc, arena=(5.0, 4.0))
    for B in (2, 257, 2048):
        c[f"dense_B{B}"] = dict(poses=dp, circles=dc, arena=(30.0, 30.0), n_beams=B)
    near = dc[np.argsort(np.hypot(dc[:, 0], dc[:, 1]))]  # the nearest are seen from the origin
    for n in (0, 1, 65):
        c[f"C{n}"] = dict(poses=dp, circles=near[:n], arena=(30.0, 30.0))
    for S in (1, 65):
        c[f"S{S}"] = dict(poses=_drive(S), circles=np.array(BASIC))
    scenes, pick = _per_scan_scenes(40)
    c["scenes40"] = dict(poses=_drive(40), circles=scenes, scene=pick)
    return c


CASE_NAMES = (["drive40", "lidar_world40"] + [f"dense_B{B}" for B in (2, 257, 2048)] +
              [f"C{n}" for n in (0, 1, 65)] + ["S1", "S65", "scenes40"])


def _grazing(poses, circles, scene=None, n_beams=360, **_):
    """Beams where the restatement's |disc| < 1e-9 m² for some cylinder (synth.lidar_scans_counter's
    own expressions)."""
    poses = np.atleast_2d(poses)
    circ = np.asarray(circles, dtype=np.float64)
    circ = circ.reshape((1, -1, 3)) if circ.ndim < 3 else circ
    mine = circ[np.zeros(len(poses), np.intp) if scene is None else np.asarray(scene, np.intp)]
    th = poses[:, 0:1] + np.arange(n_beams)[None, :] * (2.0 * math.pi / n_beams)
    lx = (poses[:, 1] - 0.032 * np.cos(poses[:, 0]))[:, None]
    ly = (poses[:, 2] - 0.032 * np.sin(poses[:, 0]))[:, None]
    dx, dy = np.cos(th), np.sin(th)
    graze = np.zeros(th.shape, bool)
    for c in range(mine.shape[1]):
        fx, fy, r = lx - mine[:, c, 0:1], ly - mine[:, c, 1:2], mine[:, c, 2:3]
        bq = fx * dx + fy * dy
        graze |= np.abs(bq * bq - (fx * fx + fy * fy - r * r)) < 1e-9
    return graze


@pytest.mark.parametrize("sigma", [0.0, 1e-3])
@pytest.mark.parametrize("name", CASE_NAMES)
def test_ranges_match_restatement(det, name, sigma):
    from pyekf import synth
    assert list(_cases()) == CASE_NAMES
    kw = _cases()[name]
    want = synth.lidar_scans_counter(sigma=sigma, seed=77, scan0=5, **kw)
    got = det.simulate(sigma=sigma, seed=77, scan0=5, **kw)
    assert got.shape == want.shape and got.dtype == np.float32
    skip = _grazing(**kw)
    step = np.abs(got.astype(np.float64) - want.astype(np.float64)) / np.spacing(want)
    print(f"{name} σ={sigma}: {skip.sum()} of {skip.size} beams grazing, "
          f"{(step[~skip] > 0).sum()} a step off, worst {step[~skip].max():.2f} steps")
    assert skip.sum() <= 0.005 * skip.size
    assert np.isfinite(got).all()
    assert (step[~skip] <= 1.0).all()
    if sigma == 0.0 and kw["circles"].size and want.shape[1] > 2:  # the case sees its cylinders
        walls = synth.lidar_scans_counter(kw["poses"], [], arena=kw.get("arena", (10.0, 5.0)),
                                          n_beams=want.shape[1])
        assert (want < walls).any()


def test_clamp_to_range_max(det):
    got = det.simulate(_drive(5), [], arena=(30.0, 30.0))
    assert (got.view(np.uint32) == np.float32(10.0).view(np.uint32)).all()


def test_clamp_to_range_min(det):
    th, x, y = 0.7, 0.3, -0.2
    lx, ly = x - 0.032 * math.cos(th), y - 0.032 * math.sin(th)
    circle = [(lx + 0.1 * math.cos(th), ly + 0.1 * math.sin(th), 0.03)]  # hit at 0.07 m < 0.11
    got = det.simulate([(th, x, y)], circle)
    assert got[0, 0].view(np.uint32) == np.float32(0.11).view(np.uint32)
    assert got[0, 180] > 1.0


def test_deterministic_and_split_by_scan0(det):
    poses, circles = _drive(40), np.array(BASIC)
    a = det.simulate(poses, circles, sigma=1e-3, seed=3)
    b = det.simulate(poses, circles, sigma=1e-3, seed=3)
    np.testing.assert_array_equal(a.view(np.uint32), b.view(np.uint32))
    assert (a != det.simulate(poses, circles, sigma=1e-3, seed=4)).mean() > 0.9
    for k in (1, 17):
        head = det.simulate(poses[:k], circles, sigma=1e-3, seed=3)
        tail = det.simulate(poses[k:], circles, sigma=1e-3, seed=3, scan0=k)
        np.testing.assert_array_equal(np.concatenate([head, tail]).view(np.uint32),
                                      a.view(np.uint32))


def _same_markers(cnt, mk, cnt2, mk2):
    np.testing.assert_array_equal(cnt, cnt2)
    for s in range(len(cnt)):
        k = max(int(cnt[s]), 0)
        assert mk[s, :k].tobytes() == mk2[s, :k].tobytes()


@pytest.mark.parametrize("name", ["drive40", "lidar_world40"])
def test_detect_resident_is_detect_on_the_same_scans(det, name):
    scans = det.simulate(sigma=1e-3, seed=11, **_cases()[name])
    cnt, mk = det.detect_resident()
    cnt2, mk2 = det.detect_resident()  # the scans stay resident
    _same_markers(cnt, mk, cnt2, mk2)
    T = len(scans)
    cnt3, mk3 = det.detect(scans, np.zeros(T), np.full(T, INC360))
    _same_markers(cnt, mk, cnt3, mk3)
    assert cnt.sum() >= 20
    for t in range(T):
        want = L.laser_callback(scans[t], 0.0, INC360)
        assert cnt[t] == len(want)
        got = np.array([[m["x"], m["y"]] for m in mk[t, :cnt[t]]]).reshape(-1, 2)
        ref = np.array([[w[1], w[2]] for w in want]).reshape(-1, 2)
        assert np.abs(got - ref).max(initial=0.0) < 1e-9


def test_detect_resident_without_host_ranges(det):
    """ranges=False: nothing comes back from simulate, and detection sees the same scans."""
    kw = _cases()["scenes40"]
    scans = det.simulate(sigma=1e-3, seed=2, **kw)
    cnt, mk = det.detect_resident()
    assert det.simulate(sigma=1e-3, seed=2, ranges=False, **kw) is None
    assert det.last_simulate_us() > 0.0  # waits for the kernel the call left in flight
    cnt2, mk2 = det.detect_resident()
    _same_markers(cnt, mk, cnt2, mk2)
    assert cnt.sum() >= 20 and scans.shape == (40, 360)
    assert det.last_simulate_us() > 0.0


def test_device_scan_to_posterior_matches_oracles(det):
    """test_gpu_pipeline.test_scan_to_posterior_matches_oracles with the scans made on the device:
    lm_simulate → lm_detect_resident → ekf_sensor against laser_callback → OracleEKF.sensor_cb on
    the same device scans."""
    import pyekf
    T = 40
    poses = _drive(T)
    scans = det.simulate(poses, BASIC, sigma=0.001, seed=11)
    cnt, mk = det.detect_resident()
    ekf = pyekf.EKF(n_landmarks=50)
    ref = orc.OracleEKF(n_landmarks=50)
    seen = 0
    for t in range(T):
        want = L.laser_callback(scans[t], 0.0, INC360)
        assert cnt[t] == len(want)
        got = np.array([[m["x"], m["y"]] for m in mk[t, :cnt[t]]]).reshape(-1, 2)
        ref_xy = np.array([[w[1], w[2]] for w in want]).reshape(-1, 2)
        assert np.abs(got - ref_xy).max(initial=0.0) < 1e-9
        ekf.set_odom(poses[t])
        ref.set_odom(poses[t])
        if cnt[t] == 0:
            continue
        seen += int(cnt[t])
        rc, j, nw = ekf.sensor(got)
        rrc, rj, rnw = ref.sensor_cb(ref_xy)
        assert rc == rrc == 0
        np.testing.assert_array_equal(j, rj)
        np.testing.assert_array_equal(nw, rnw)
        x = ekf.pose()
        xr = ref.get(sigma=False)[0][:3]
        assert np.abs(x - xr).max() < 1e-8, (t, x - xr)
    assert seen >= 20
    ekf.close()


def test_bad_arguments_are_rejected_and_the_handle_survives():
    import pyekf
    from pyekf import synth
    from pyekf.landmarks import MARKER_DTYPE, Detector
    lib = pyekf.lib()
    d = Detector(max_scans=8, max_beams=360)
    cfg = pyekf.ScanConfig()
    lib.lm_scan_config_default(C.byref(cfg))
    assert (cfg.scan0, cfg.arena_w, cfg.arena_h, cfg.range_min, cfg.range_max, cfg.sigma) == \
        (0, 10.0, 5.0, 0.11, 10.0, 0.0)
    poses = np.ascontiguousarray(_drive(8))
    circ = np.ascontiguousarray(np.array(BASIC))
    big = np.zeros((1025, 3))
    out = np.zeros((8, 360), np.float32)
    mk = np.zeros((8, 4), MARKER_DTYPE)
    cnt = np.zeros(8, np.int32)
    us = C.c_double()

    def sim(S=8, B=360, p=poses, G=1, Cn=4, c=circ, scene=None, k=cfg, h=d.h):
        return lib.lm_simulate(h, S, B, None if p is None else p.ctypes.data, G, Cn,
                               None if c is None else c.ctypes.data,
                               None if scene is None else scene.ctypes.data,
                               None if k is None else C.byref(k), out.ctypes.data)

    E = pyekf.EKF_E_ARG
    # nothing resident yet
    assert lib.lm_detect_resident(d.h, 0.2, mk.ctypes.data, 4, cnt.ctypes.data) == E
    assert lib.lm_last_simulate_us(d.h, C.byref(us)) == E
    assert sim(h=None) == E
    assert sim(S=9) == E and sim(S=0) == E                       # S outside [1, max_scans]
    assert sim(B=1) == E and sim(B=361) == E                     # B outside [2, max_beams]
    assert sim(Cn=1025, c=big) == E and sim(Cn=-1) == E          # C outside [0, LM_MAX_CIRCLES]
    assert sim(G=0) == E
    for bad in (1, -1):
        scene = np.zeros(8, np.int32)
        scene[5] = bad
        assert sim(scene=scene) == E                             # a scene index outside [0, G)
    assert sim(p=None) == E and sim(k=None) == E and sim(c=None) == E
    assert lib.lm_detect_resident(d.h, 0.2, mk.ctypes.data, 4, cnt.ctypes.data) == E
    # the handle still works, walls only with no circle pointer included
    assert sim(Cn=0, c=None) == pyekf.EKF_OK
    np.testing.assert_array_equal(out, synth.lidar_scans_counter(poses, []))
    want = synth.lidar_scans_counter(poses, BASIC)
    assert sim() == pyekf.EKF_OK
    assert (np.abs(out - want) <= np.spacing(want)).mean() > 0.995
    assert lib.lm_last_simulate_us(d.h, C.byref(us)) == pyekf.EKF_OK and us.value > 0.0
    # resident detection: argument checks, then a rejected simulate keeps the resident scans
    assert lib.lm_detect_resident(d.h, 0.2, mk.ctypes.data, 4, None) == E
    assert lib.lm_detect_resident(d.h, 0.2, None, 4, cnt.ctypes.data) == E
    assert lib.lm_detect_resident(d.h, 0.2, mk.ctypes.data, -1, cnt.ctypes.data) == E
    assert sim(S=9) == E
    assert lib.lm_detect_resident(d.h, 0.2, mk.ctypes.data, 4, cnt.ctypes.data) == pyekf.EKF_OK
    first = cnt.copy()
    # a host lm_detect overwrites the range buffer: nothing is resident after it
    cnt2, _ = d.detect(out, np.zeros(8), np.full(8, INC360), max_markers=4)
    np.testing.assert_array_equal(cnt2, first)
    assert lib.lm_detect_resident(d.h, 0.2, mk.ctypes.data, 4, cnt.ctypes.data) == E
    assert sim() == pyekf.EKF_OK
    assert lib.lm_detect_resident(d.h, 0.2, mk.ctypes.data, 4, cnt.ctypes.data) == pyekf.EKF_OK
    np.testing.assert_array_equal(cnt, first)
    d.close()
