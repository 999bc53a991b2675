"""synth.lidar_scans_counter, the host restatement of the device's simulated laser (lm_simulate):
lidar_scans' geometry with per-scan scenes and the counter-based RNG. No GPU needed."""
import math

import numpy as np
import pytest

from pyekf import synth

BASIC = [(-0.5, -0.7, 0.038), (0.8, -0.8, 0.038), (0.4, 0.8, 0.038), (-0.6, 0.65, 0.038)]


def _drive(T):
    """tests/test_gpu_pipeline._drive: a circle of radius 0.5 m about (0.1, 0), 0.1 rad a message."""
    return np.array([(0.1 * t + math.pi / 2, 0.1 + 0.5 * math.cos(0.1 * t),
                      0.5 * math.sin(0.1 * t)) for t in range(T)])


def _bits(a):
    assert a.dtype == np.float32
    return a.view(np.uint32)


def test_noiseless_is_lidar_scans_bit_for_bit():
    poses = _drive(40)
    want = synth.lidar_scans(poses, BASIC)
    got = synth.lidar_scans_counter(poses, BASIC, sigma=0.0)
    assert got.shape == (40, 360)
    np.testing.assert_array_equal(_bits(got), _bits(want))
    # the scans are not trivial: cylinders are hit and walls are seen
    assert (want < 1.0).sum() > 100 and (want > 2.0).sum() > 1000


def test_same_seed_same_bits_other_seed_other_noise():
    poses = _drive(8)
    a = synth.lidar_scans_counter(poses, BASIC, sigma=1e-3, seed=5)
    b = synth.lidar_scans_counter(poses, BASIC, sigma=1e-3, seed=5)
    c = synth.lidar_scans_counter(poses, BASIC, sigma=1e-3, seed=6)
    np.testing.assert_array_equal(_bits(a), _bits(b))
    assert (a != c).mean() > 0.9


@pytest.mark.parametrize("k", [1, 7, 12])
def test_split_at_scan0_equals_one_call(k):
    poses = _drive(13)
    whole = synth.lidar_scans_counter(poses, BASIC, sigma=1e-3, seed=9, scan0=3)
    head = synth.lidar_scans_counter(poses[:k], BASIC, sigma=1e-3, seed=9, scan0=3)
    tail = synth.lidar_scans_counter(poses[k:], BASIC, sigma=1e-3, seed=9, scan0=3 + k)
    np.testing.assert_array_equal(_bits(np.concatenate([head, tail])), _bits(whole))


def test_per_scan_scenes_select_their_circles():
    poses = _drive(6)
    rng = np.random.default_rng(3)
    scenes = np.zeros((3, 4, 3))
    for g in range(3):
        scenes[g] = np.asarray(BASIC) + np.r_[rng.uniform(-0.05, 0.05, 2), 0.0]
    pick = np.array([2, 0, 1, 1, 2, 0])
    got = synth.lidar_scans_counter(poses, scenes, scene=pick, sigma=1e-3, seed=4)
    for s in range(6):
        one = synth.lidar_scans_counter(poses[s], scenes[pick[s]], sigma=1e-3, seed=4, scan0=s)
        np.testing.assert_array_equal(_bits(got[s:s + 1]), _bits(one))
    # and the scenes do differ: scan 0 under scene 0 is another scan
    other = synth.lidar_scans_counter(poses[0], scenes[0], sigma=1e-3, seed=4)
    assert (other != got[0:1]).any()
    with pytest.raises(ValueError):
        synth.lidar_scans_counter(poses, scenes, scene=np.array([0, 1, 2, 3, 0, 0]))
    with pytest.raises(ValueError):
        synth.lidar_scans_counter(poses, scenes, scene=np.array([0, 1]))


def test_no_circles_is_walls_only():
    got = synth.lidar_scans_counter([(0.3, 0.2, -0.1)], [])
    want = synth.lidar_scans([(0.3, 0.2, -0.1)], [])
    np.testing.assert_array_equal(_bits(got), _bits(want))


def test_noise_moments():
    """10⁵ draws (278 scans × 360 beams of an empty 30 × 30 arena: every noiseless range is the
    10 m clamp): |mean| < 4σ/√n, standard deviation within 2 % of σ. σ = 0.5 m keeps float32's
    rounding at 10 m (5·10⁻⁷) five orders below the bounds."""
    sigma = 0.5
    r = synth.lidar_scans_counter(np.zeros((278, 3)), [], arena=(30.0, 30.0), sigma=sigma, seed=1)
    d = r.astype(np.float64) - 10.0
    n = d.size
    assert n >= 100000
    assert abs(d.mean()) < 4.0 * sigma / math.sqrt(n)
    assert abs(d.std() / sigma - 1.0) < 0.02
