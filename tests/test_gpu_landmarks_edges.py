"""The landmark front-end at wave edges, size limits and dense scans: the inputs of
tests/frontend_scans.py (pinned on the CPU by tests/test_frontend_scans.py) through lm_detect,
lm_detect_device / lm_fetch_markers, lm_fit_circles and lm_check_circles, against the numpy oracle.

Tolerances are those of tests/test_gpu_landmarks.py: counts, ids and check_circle decisions exactly;
x, y, r of detected markers within 1e-9 m; direct fits within rtol = atol = 1e-9.

The fits are compared at point noise σ ∈ {1e-5 … 1e-8} and {1e-13, 1e-14, 0}, on both sides of the
band of about 1e-12 m to 3e-9 m in which the reference's Hyper fit is itself ill-determined in
double precision (s_min(Z) is above the 1e-11 branch threshold while s_min² is below the rounding of
Q = Y·H⁻¹·Y, so eig_sym's eigenvector is arbitrary): parity with the oracle is neither expected nor
tested there ("The ill-determined band"). Real and simulated scans sit above it:
the float32 quantisation of a range alone is about 1e-8 m.
"""
import functools
import math

import numpy as np
import pytest

import frontend_scans as F
import landmarks_numpy as L

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def det():
    from pyekf.landmarks import Detector
    d = Detector(max_scans=130, max_beams=2048)
    yield d
    d.close()


def _detect(det, cases, max_markers=32):
    assert len({c.n_beams for c in cases}) == 1
    return det.detect(np.stack([c.ranges for c in cases]), [c.angle_min for c in cases],
                      [c.angle_inc for c in cases], max_markers=max_markers)


def _assert_rows(cnt, mk, cases, max_markers, what):
    """Counts and ids exactly, x, y, r within 1e-9 m of the oracle's laser_callback; the rows are
    its first ``max_markers`` markers. Returns the valid-row mask."""
    ecnt, ids, xyr, valid = F.expected_rows(cases, max_markers)
    assert np.array_equal(cnt, ecnt), (what, [c.name for c, a, b in zip(cases, cnt, ecnt) if a != b])
    assert np.array_equal(mk["id"][valid], ids[valid]), what
    assert not mk["pad"][valid].any()
    got = np.stack([mk["x"], mk["y"], mk["r"]], -1)
    err = np.abs(got - xyr)[valid]
    print(f"{what}: {len(cases)} scans, {int(valid.sum())} markers, "
          f"worst |Δ| {err.max() if err.size else 0.0:.2e}")
    assert np.allclose(got[valid], xyr[valid], rtol=0, atol=1e-9), (what, err.max())
    return valid


# ---------------------------------------------------------------------- detect, one scan at a time

@pytest.mark.parametrize("family", list(F.FAMILIES))
def test_detect_single_scans(det, family):
    mm = 128 if family == "dense_ring" else 32
    for c in F.FAMILIES[family]():
        cnt, mk = _detect(det, [c], mm)
        _assert_rows(cnt, mk, [c], mm, c.name)


@pytest.mark.parametrize("max_markers", [32, 64, 65])
def test_dense_ring_beyond_the_marker_capacity(det, max_markers):
    """The count is the full count; the rows are the oracle's first max_markers markers."""
    for c in F.dense_ring()[:3]:
        cnt, mk = _detect(det, [c], max_markers)
        assert cnt[0] == len(F.oracle(c)) > max_markers
        valid = _assert_rows(cnt, mk, [c], max_markers, f"{c.name}/{max_markers}")
        assert valid.all()


# ------------------------------------------------------------------------------------- batches

@pytest.mark.parametrize("S", [1, 63, 64, 65, 130])
def test_batches_of_mixed_scans(det, S):
    """Size limits, the turned scene and no-break rooms interleaved, angle_min per scan: row s is
    the oracle's result for scan s."""
    cases = F.batch_cases()[:S]
    cnt, mk = _detect(det, cases)
    _assert_rows(cnt, mk, cases, 32, f"batch S={S}")


def test_handle_reuse_across_batch_and_beam_sizes(det):
    big = F.batch_cases()
    cnt0, mk0 = _detect(det, big)
    v0 = _assert_rows(cnt0, mk0, big, 32, "S=130, B=360")
    ring = [F.dense_ring()[1]]
    cnt, mk = _detect(det, ring, 128)
    _assert_rows(cnt, mk, ring, 128, "S=1, B=2048")
    small = F.small_batch()
    cnt, mk = _detect(det, small)
    _assert_rows(cnt, mk, small, 32, "S=3, B=65")
    cnt1, mk1 = _detect(det, big)
    v1 = _assert_rows(cnt1, mk1, big, 32, "S=130, B=360 again")
    assert cnt0.tobytes() == cnt1.tobytes()
    assert np.array_equal(v0, v1) and mk0[v0].tobytes() == mk1[v1].tobytes()  # (slots past the
    # count are not written)


# --------------------------------------------------------------------------------- device path

def test_device_markers_fetched_whole_and_pitched(det):
    cases = F.batch_cases()[:65]
    cnt, mk = _detect(det, cases)
    valid = _assert_rows(cnt, mk, cases, 32, "detect S=65")
    assert cnt.max() == 3
    S = det.detect_device(np.stack([c.ranges for c in cases]), [c.angle_min for c in cases],
                          [c.angle_inc for c in cases], max_markers=32)
    assert S == 65
    c_full, m_full = det.fetch_markers(32)
    assert np.array_equal(c_full, cnt) and m_full[valid].tobytes() == mk[valid].tobytes()
    c_cut, m_cut = det.fetch_markers(2)   # narrower than the device rows: the pitched copy
    assert m_cut.shape == (65, 2) and np.array_equal(c_cut, cnt)   # the count stays the full count
    assert m_cut[valid[:, :2]].tobytes() == mk[:, :2][valid[:, :2]].tobytes()
    _assert_rows(c_cut, m_cut, cases, 2, "fetch_markers(2)")


# ----------------------------------------------------------------------- direct fits and checks

@functools.lru_cache(maxsize=None)
def _arcs(sigma):
    arcs, dropped = F.fit_arcs(sigma, 200, seed=11)
    fits = np.array([L.fit_circle(a) for a in arcs])
    checks = np.array([L.check_circle(a) for a in arcs])
    return arcs, fits, checks, dropped


def _assert_fits(got, want, what):
    err = np.abs(got - want)
    print(f"{what}: {len(want)} clusters, worst |Δ| {err.max():.2e}")
    assert np.allclose(got, want, rtol=1e-9, atol=1e-9), (what, err.max())


@pytest.mark.parametrize("sigma", F.FIT_SIGMAS)
def test_fit_and_check_at_noise_level(det, sigma):
    arcs, fits, checks, _ = _arcs(sigma)
    _assert_fits(det.fit_circles(arcs), fits, f"fit σ={sigma:g}")
    assert 20 < checks.sum() < len(arcs) - 20
    assert np.array_equal(det.check_circles(arcs), checks)


def test_fit_levels_drop_few_arcs():
    dropped = sum(_arcs(s)[3] for s in F.FIT_SIGMAS)
    print(f"dropped {dropped} of {200 * len(F.FIT_SIGMAS)} arcs inside the ill-determined band")
    assert dropped <= 0.02 * 200 * len(F.FIT_SIGMAS)


def test_three_point_fit_is_the_circumcircle(det):
    """n = 3: Z has rank 3, the null-vector branch gives the circle through the points. (The
    oracle's economy SVD has no fourth right vector at n = 3, so it cannot be the reference.)"""
    cl, drawn = F.triples(300, seed=13)
    want = np.array([F.circumcircle(p) for p in cl])
    assert np.allclose(want, drawn, rtol=0, atol=1e-12)
    got = det.fit_circles(cl)
    err = np.abs(got - want)
    print(f"three-point fit: 300 clusters, worst |Δ| {err.max():.2e}")
    assert np.allclose(got, want, rtol=0, atol=1e-9), err.max()


def test_check_small_and_repeated_point_clusters(det):
    rng = np.random.default_rng(17)
    cl = []
    for n in (3, 4, 5):
        for _ in range(40):
            a = F.random_arc(rng, 1e-3)
            cl.append(a[np.sort(rng.choice(len(a), n, replace=False))])
    n_plain = len(cl)
    for _ in range(20):   # an interior point on an end point: a NaN angle
        a = F.random_arc(rng, 0.0)
        a[1] = a[0]
        cl.append(a)
        b = F.random_arc(rng, 0.0)
        b[-2] = b[-1]
        cl.append(b)
    want = np.array([L.check_circle(c) for c in cl])
    assert 10 < want[:n_plain].sum() < n_plain - 10 and not want[n_plain:].any()
    assert np.array_equal(det.check_circles(cl), want)


@pytest.mark.parametrize("nc", [1, 63, 64, 65, 129])
def test_fit_and_check_cluster_counts(det, nc):
    arcs, fits, checks, _ = _arcs(1e-5)
    _assert_fits(det.fit_circles(arcs[:nc]), fits[:nc], f"fit nc={nc}")
    assert np.array_equal(det.check_circles(arcs[:nc]), checks[:nc])


def test_staging_grows_on_demand():
    """nc = 1, 129, 5 on a fresh handle: the staging buffers grow, then serve a smaller call."""
    from pyekf.landmarks import Detector
    arcs, fits, checks, _ = _arcs(1e-6)
    d = Detector(max_scans=1, max_beams=64)
    try:
        for lo, hi in ((0, 1), (1, 130), (130, 135)):
            _assert_fits(d.fit_circles(arcs[lo:hi]), fits[lo:hi], f"fit [{lo}, {hi})")
            assert np.array_equal(d.check_circles(arcs[lo:hi]), checks[lo:hi])
    finally:
        d.close()


def test_degenerate_fits_leave_the_handle_usable(det):
    """A collinear cluster, identical points, one point, two points: lm_fit_circles returns EKF_OK
    (fit_circles raises otherwise) with a non-finite circle, and the next fit is correct."""
    # coordinates that are binary fractions: the means are exact, so the centred cluster is the
    # degenerate one exactly (six copies of 0.7 average to 0.7 less an ulp, and the "cluster" is
    # then a cloud of rounding errors with a finite, meaningless fit, on the oracle as well)
    x = np.arange(-4, 5) / 16.0
    bad = [np.stack([1.0 + x, np.full(9, 0.5)], 1),        # collinear
           np.tile([[0.75, -0.25]], (6, 1)),               # identical
           np.array([[0.375, 0.5]]),                       # n = 1
           np.array([[0.25, 0.5], [0.25, 1.0]])]           # n = 2
    got = det.fit_circles(bad)
    print("degenerate fits:", got.tolist())
    assert got.shape == (4, 3)
    for k, row in enumerate(got):
        assert not np.isfinite(row).all(), (k, row)
    arcs, fits, _, _ = _arcs(1e-5)
    _assert_fits(det.fit_circles(arcs[:7]), fits[:7], "fit after the degenerate clusters")
    mixed = det.fit_circles([arcs[0], bad[1], arcs[1]])     # a lane beside a degenerate one
    _assert_fits(mixed[[0, 2]], fits[:2], "fit beside a degenerate cluster")
