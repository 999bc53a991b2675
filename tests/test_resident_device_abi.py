"""ekf_replay_resident and lm_replay_resident (include/ekf.h, include/landmarks.h) without a GPU:
the library exports them, pyekf lists them, and a NULL handle is refused before anything else."""
import pyekf

NEW = ("ekf_replay_resident", "lm_replay_resident")


def test_symbols_exported_and_listed():
    lib = pyekf.lib()
    for name in NEW:
        assert hasattr(lib, name), name
        assert name in pyekf.EXPORTS
        assert pyekf.EXPORTS.count(name) == 1


def test_null_handles_are_refused():
    lib = pyekf.lib()
    assert lib.ekf_replay_resident(None, 0, 1, 1, None, None, None, None, 2, None) == pyekf.EKF_E_ARG
    assert lib.ekf_replay_resident(None, 1, 4, 16, None, None, None, None, 4, None) == pyekf.EKF_E_ARG
    assert lib.lm_replay_resident(None, None, 1, None) == pyekf.EKF_E_ARG


def test_python_surface():
    for name in ("replay_resident", "replay_resident_raw", "replay_on_device"):
        assert callable(getattr(pyekf.EKF, name))
    from pyekf.landmarks import Detector
    assert callable(Detector.replay_resident)
