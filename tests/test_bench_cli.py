"""bench.py's command line on the CPU (the C oracle injected as the backend, one rank): a plain run
prints the headline line alone, --full adds the legs beside it, and --dump-outputs writes what the
timed steps computed, the same from run to run and with or without --full.
"""
import os
import sys

import numpy as np

from test_multirank import TINY, CpuBackend, OracleSwarm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
HEADLINE = {"metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "steps", "warmup"}
FULL_ONLY = {"roofline", "parity", "cpu_baseline"}


def _run(tmp_path, name, *extra):
    import bench
    bench.WORKLOADS["tiny"] = TINY
    out = tmp_path / name
    args = bench.parse(["--workload", "tiny", "--gpus", "1", "--steps", "3", "--warmup", "2",
                        "--dump-outputs", str(out), *extra])
    result, poses = bench.run(args, 0, 1, 0, CpuBackend())
    return result, poses, {f[:-4]: np.load(out / f) for f in sorted(os.listdir(out))}


def test_plain_run_is_lean_and_full_adds_the_legs(tmp_path, capsys):
    plain, poses, dumped = _run(tmp_path, "plain")
    lines = [ln for ln in capsys.readouterr().out.splitlines() if ln.strip()]
    assert len(lines) == 1 and lines[0].startswith("{")  # one JSON result line
    assert HEADLINE <= set(plain) and not FULL_ONLY & set(plain)
    assert plain["steps"] == 3 and plain["warmup"] == 2 and plain["ms_per_step"] > 0
    full, poses_f, dumped_f = _run(tmp_path, "full", "--full", "--traffic", "off",
                                   "--parity-messages", "2")
    assert HEADLINE | FULL_ONLY <= set(full)
    assert full["parity"]["pose_rmse_m"] == 0.0
    for k in ("metric", "unit", "higher_is_better", "dtype", "steps", "warmup"):
        assert plain[k] == full[k]
    # the extra legs run after the dump: both runs wrote the same arrays
    assert sorted(dumped) == sorted(dumped_f) == ["poses", "sampled_filters", "sigma", "state"]
    for k in dumped:
        np.testing.assert_array_equal(dumped[k], dumped_f[k])
    np.testing.assert_array_equal(poses, poses_f)


def test_dump_outputs_is_the_state_after_the_timed_steps(tmp_path):
    import bench
    _, poses, dumped = _run(tmp_path, "d")
    N, _, F, m, _ = TINY
    n = 3 + 2 * N
    assert all(a.dtype == np.float64 for a in dumped.values())
    assert dumped["poses"].shape == (F, 3) and dumped["state"].shape == (F, n)
    assert dumped["sigma"].shape == (F, n, n)
    np.testing.assert_array_equal(dumped["sampled_filters"], np.arange(F))
    np.testing.assert_array_equal(dumped["poses"], poses)
    np.testing.assert_array_equal(dumped["state"][:, :3], poses)
    # the same messages through a fresh oracle swarm: survey, 2 warm-up and 3 timed messages
    sw, odom, _ = bench.build_inputs(N, F, 2 + 2 * 3, 20240317, m, 0)
    T = sw.n_warm + 2 + 3
    ref = OracleSwarm(N, F)
    ref.replay(sw.count[:T], sw.rel[:T], odom[:T], ids=sw.ids[:T], actions=sw.actions[:T])
    for f in range(F):
        x, S, _ = ref.state(f)
        np.testing.assert_array_equal(dumped["state"][f], x)
        np.testing.assert_array_equal(dumped["sigma"][f], S)


def test_dump_sample_is_fixed_and_bounded():
    import bench
    n = 3 + 2 * 256
    a, b = bench.dump_filters(512, n), bench.dump_filters(512, n)
    np.testing.assert_array_equal(a, b)
    assert len(set(a.tolist())) == len(a) and a.min() >= 0 and a.max() < 512
    assert np.all(np.diff(a) > 0)
    # Σ, state, poses of every filter and the sample's indices stay under 64 MB
    assert len(a) * (n * n + n + 1) * 8 + 512 * 3 * 8 <= 64e6
    np.testing.assert_array_equal(bench.dump_filters(1, 3 + 2 * 1024), [0])
    assert (3 + 2 * 1024) ** 2 * 8 + (3 + 2 * 1024) * 8 + 32 <= 64e6
