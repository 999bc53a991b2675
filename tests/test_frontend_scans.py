"""The front-end's edge inputs (tests/frontend_scans.py) reach what they claim, on the oracle alone:
so that the GPU tests that run them (tests/test_gpu_landmarks_edges.py) can neither pass vacuously
nor fail through an ill-determined reference."""
import math

import numpy as np
import pytest

import frontend_scans as F
import landmarks_numpy as L


def test_case_names_are_unique():
    names = [c.name for c in F.all_cases() + F.rooms()]
    assert len(names) == len(set(names))
    assert all(c.ranges.dtype == np.float32 and not c.ranges.flags.writeable
               for c in F.all_cases())


def test_dense_ring_fills_several_marker_chunks():
    for c, (n_cand, n_mark, top) in zip(F.dense_ring(), F.RING_COUNTS):
        assert c.n_beams == 2048
        cl = L.get_clusters(c.ranges, c.angle_min, c.angle_inc)
        cand = [k for k in cl if 3 < len(k) < 40]
        assert len(cand) == n_cand > 128                 # ≥ three iterations of k_markers' loop
        m = F.oracle(c)
        assert len(m) == n_mark and m[-1][0] == top > 65
        # passing and failing candidates alternate in every full 64-candidate chunk
        ok = [L.check_circle(k) for k in cand]
        for cb in range(0, n_cand - 63, 64):
            assert 10 < sum(ok[cb:cb + 64]) < 54
    assert all(len(F.oracle(c)) > 65 for c in F.dense_ring()[:3])   # max_markers 32, 64, 65 cut
    far = F.oracle(F.dense_ring()[3])   # circles beyond 2 m take an id and no slot
    assert [k for k, *_ in far] == list(range(1, 99, 2))


def test_size_limits_hit_each_size_plain_and_merged():
    seen = set()
    for c in F.size_limits():
        _, kind, n = c.name.split("_")
        n = int(n)
        cl = L.get_clusters(c.ranges, c.angle_min, c.angle_inc)
        sizes, merged = F.cluster_sizes(c)
        assert merged
        if kind == "merged":
            hit = cl[:1]
            # two runs: cluster 0 holds beams from both ends of the scan
            br = F.break_indices(c)
            assert (br[0], c.n_beams - br[-1] - 1) == F.SIZE_MERGED[n] and sum(F.SIZE_MERGED[n]) == n
        else:
            hit = [k for k in cl[1:] if len(k) == n and L.check_circle(k)]
        # the cluster is a circle by check_circle: only the size gate keeps 3 and 40 out
        assert len(hit) == 1 and len(hit[0]) == n and L.check_circle(hit[0])
        assert sum(L.check_circle(k) for k in cl if len(k) > 2) == 1
        assert len(F.oracle(c)) == (1 if n in (4, 39) else 0)
        seen.add((kind, n))
    assert seen == {(k, n) for k in ("plain", "merged") for n in (3, 4, 39, 40)}


def test_chunk_edges_breaks_cover_the_chunk_boundaries():
    cases = F.chunk_edges()
    assert len(cases) == 64 and all(c.n_beams == 360 for c in cases)
    br = [F.break_indices(c) for c in cases]
    assert {i % 64 for b in br for i in b} >= {0, 1, 62, 63}
    assert {i for b in br for i in b} >= {1, 63, 64, 65, 127, 128, 129, 359}
    assert all(F.oracle(c) for c in cases)   # every turn of the scene yields markers


def test_odd_beams_and_written_scans():
    cases = {c.name: c for c in F.odd_beams()}
    for B in F.ODD_BEAMS:
        c = cases[f"odd_beams_{B}"]
        assert c.n_beams == B and c.angle_inc == float(np.float32(2.0 * math.pi / B))
        assert len(F.oracle(c)) >= 1
    want = {"2_break": (1, 0), "2_room": (0, None), "3_break": (1, 0), "3_room": (0, None),
            "5_break": (2, 0), "5_first": (1, 0), "5_room": (0, None)}
    for name, (nb, count) in want.items():
        c = cases[f"odd_beams_{name}"]
        assert c.n_beams == int(name[0])
        assert len(F.break_indices(c)) == nb
        m = F.oracle(c)
        assert (m is None) if count is None else (len(m) == count)
    assert F.break_indices(cases["odd_beams_5_first"]) == [1]
    assert F.break_indices(cases["odd_beams_3_break"]) == [2]


def test_degenerate_patterns():
    c = {x.name[len("degenerate_"):]: x for x in F.degenerate()}
    for B in (2048, 65):
        a = c[f"alternating_{B}"]
        assert F.break_indices(a) == list(range(1, B))
        sizes, merged = F.cluster_sizes(a)
        assert merged == (B == 65) and F.oracle(a) == ()
        assert sizes[0] == 1 and not any(sizes[1:])
    assert F.break_indices(c["far_beam_mid"]) == [180, 181]
    assert F.cluster_sizes(c["far_beam_mid"]) == ([358, 0], True)
    assert F.break_indices(c["one_break_open"]) == [359]
    assert F.cluster_sizes(c["one_break_open"]) == ([359, 0], False)
    assert F.break_indices(c["one_break_merged"]) == [180]
    assert F.cluster_sizes(c["one_break_merged"]) == ([359], True)
    assert np.isnan(c["nan_first"].ranges[0]) and 1 in F.break_indices(c["nan_first"])
    assert np.isnan(c["nan_last"].ranges[-1]) and 359 in F.break_indices(c["nan_last"])
    assert np.isinf(c["inf_ends"].ranges[[0, -1]]).all()
    for name in ("nan_first", "nan_last", "inf_ends"):
        assert not F.cluster_sizes(c[name])[1]      # a non-finite closing distance: not merged
        assert len(F.oracle(c[name])) == 3
    assert F.break_indices(c["all_nan"]) == list(range(1, 360)) and F.oracle(c["all_nan"]) == ()
    assert all(F.oracle(r) is None for r in F.rooms())


def test_batch_mixes_rooms_sizes_and_angles():
    b = F.batch_cases()
    assert len(b) == 130 and all(c.n_beams == 360 for c in b)
    assert {c.angle_min for c in b} == {0.0, F.ANGLE_MIN_ALT}
    cnt = [None if F.oracle(c) is None else len(F.oracle(c)) for c in b]
    for S in (1, 63, 64, 65, 130):
        assert None in cnt[:max(S, 4)] and 0 in cnt[:S]
    assert {c.name for c in b} >= {c.name for c in F.size_limits()}
    assert {None, 0, 1, 2, 3} <= set(cnt)
    # the second angle_min moves every marker: the oracle is fed it, not the default
    c = next(x for x in b if x.angle_min != 0.0 and F.oracle(x))
    m0 = F.oracle(F.Case(c.name, c.ranges, 0.0, c.angle_inc))
    m1 = F.oracle(c)
    assert math.hypot(m0[0][1] - m1[0][1], m0[0][2] - m1[0][2]) > 1e-3


@pytest.mark.parametrize("family", list(F.FAMILIES) + ["batch", "small_batch"])
def test_margins(family):
    cases = {"batch": F.batch_cases, "small_batch": F.small_batch}.get(family) or F.FAMILIES[family]
    bad = {f"{c.name}@{c.angle_min}": v for c in cases() if (v := F.margin_violations(c))}
    assert not bad, bad


def test_margin_check_sees_a_violation():
    """The checker is not vacuous: a consecutive distance on the threshold and a cluster inside the
    ill-determined band are both reported."""
    # two beams along one ray whose float32 ranges differ by 0.2 m to within 1e-9
    r1 = next(v for v in np.arange(1e-3, 2e-3, 1e-6, dtype=np.float32)
              if abs(float(np.float32(v + 0.2)) - float(v) - 0.2) < 5e-10)
    on = F._case("on_threshold", [r1, np.float32(r1 + 0.2)], angle_inc=0.0)
    assert any("distance" in v for v in F.margin_violations(on))
    assert not F.margin_violations(F._case("off_threshold", [r1, r1 + 0.25], angle_inc=0.0))
    rng = np.random.default_rng(1)
    arc = F.random_arc(rng, 0.0)
    arc = arc + rng.normal(0.0, 1e-10, arc.shape)
    assert F.in_band(arc)
    assert not F.in_band(F.random_arc(rng, 0.0))
    assert not F.in_band(F.random_arc(rng, 1e-5))


# ------------------------------------------------------------------ the oracle's fit is well-determined

def mp_fit_circle(cluster, digits=60):
    """landmarks_numpy.fit_circle restated at ``digits`` decimal digits: the same Hyper fit, branch
    threshold and eigenvalue choice."""
    import mpmath
    mp = mpmath.mp
    old = mp.dps
    mp.dps = digits
    try:
        P = [(mpmath.mpf(float(x)), mpmath.mpf(float(y))) for x, y in cluster]
        n = len(P)
        mx = mpmath.fsum(p[0] for p in P) / n
        my = mpmath.fsum(p[1] for p in P) / n
        rows = [(p[0] - mx, p[1] - my) for p in P]
        z = [x * x + y * y for x, y in rows]
        z_mean = mpmath.fsum(z) / n
        Z = mpmath.matrix([[z[i], rows[i][0], rows[i][1], 1] for i in range(n)])
        H_inv = mpmath.eye(4)
        H_inv[0, 0] = 0
        H_inv[3, 0] = H_inv[0, 3] = mpmath.mpf(1) / 2
        H_inv[3, 3] = -2 * z_mean
        _, s, Vt = mp.svd_r(Z, full_matrices=False, compute_uv=True)
        V = Vt.T
        order = sorted(range(4), key=lambda i: -s[i])   # descending, like arma::svd
        s = [s[i] for i in order]
        V = mpmath.matrix([[V[r, i] for i in order] for r in range(4)])
        if min(s) < mpmath.mpf("10.0e-12"):
            A = [V[r, 3] for r in range(4)]
        else:
            Y = V * mpmath.diag(s) * V.T
            Q = Y * H_inv * Y
            Q = (Q + Q.T) / 2
            w, E = mp.eigsy(Q)
            idx, min_val = 0, mpmath.mpf("10.0e6")
            for i in sorted(range(4), key=lambda i: w[i]):   # ascending, like arma::eig_sym
                if w[i] < min_val and w[i] > 0:
                    min_val, idx = w[i], i
            A = mp.lu_solve(Y, E[:, idx])
        a = -A[1] / 2 / A[0]
        b = -A[2] / 2 / A[0]
        R = mpmath.sqrt((A[1] * A[1] + A[2] * A[2] - 4 * A[0] * A[3]) / 4 / A[0] / A[0])
        return float(a + mx), float(b + my), float(R)
    finally:
        mp.dps = old


def test_mp_fit_reproduces_a_known_answer():
    from test_landmarks import FIT_KATS
    for p, want in FIT_KATS:
        assert np.allclose(mp_fit_circle(p), want, atol=1e-4, rtol=0)


@pytest.mark.slow
def test_fit_levels_are_well_determined():
    """Outside the ill-determined band the double-precision oracle is within 1e-10 m of the same
    Hyper fit carried at 60 digits: what entitles the GPU tests to compare with the oracle at these
    noise levels (the band itself, about 1e-12 m to 3e-9 m of point noise, is not sampled)."""
    worst, dropped, total = 0.0, 0, 0
    for sigma in F.FIT_SIGMAS:
        arcs, d = F.fit_arcs(sigma, 50, seed=5)
        dropped += d
        total += 50
        for a in arcs:
            got, want = L.fit_circle(a), mp_fit_circle(a)
            err = max(abs(g - w) for g, w in zip(got, want))
            worst = max(worst, err)
            assert err < 1e-10, (sigma, len(a), err)
    print(f"worst |oracle − mp| {worst:.2e}; dropped {dropped} of {total}")
    assert dropped <= 0.02 * total
