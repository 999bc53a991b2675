"""ekf_eval_match and ekf_sim_eval_match (include/ekf.h, include/ekf_sim.h; kernel k_eval_match in
ekf-slam_amd/csrc/ekf_eval.hip) on the GPU.

The reference throughout is ekf_get_state of the same handle plus tests/match_ref.py, a numpy
restatement of the matching written operation for operation: the squared distances have the same
bits, so `match` and ekf_match_rec compare exactly. The scoring record is compared byte for byte
with what ekf_eval gives for the truth permuted into slot order by the returned `match`.

Where a frame is used the device's sin and cos are within an ulp of numpy's, so the transformed
truth differs by up to 8 eps (|x| + |y| + |x0| + |y0|), about 3e-14 m on coordinates of a few metres
(tests/test_eval_math_host.py), against distances of at least 0.05 m: the frame cases first assert
on the CPU that every seen slot's best and second-best squared distances, and its best and
max_dist^2, differ by more than 1e-9 relative, three orders above that. The matches and the counts
are then still exact; max_match_dist, a distance to a transformed point, is held to the transform's
own bound (same_record)."""
import functools

import numpy as np
import pytest

import pyekf
from pyekf import synth

import test_gpu_eval as tge
from match_ref import match_np, seen_slots, sq_distances, to_map_frame

pytestmark = pytest.mark.gpu

MAX_DIST = 0.1
MARGIN = 1e-9
FRAME = np.array([0.3, 0.5, -0.25])
UNSEEN, DUP_LO, SPUR, TIE = 7, 2, 4, 5         # slots; the duplicate's upper slot is N - 1
HANDLES = ("resident50", "f64-65", "f32-257")  # tests/test_gpu_eval.py HANDLES


# ---- crafted contents ------------------------------------------------------------------------------

def craft_slots(N, rng):
    """Slot estimates in the map frame, at least 0.4 m apart: a jittered 0.6 m grid. Slot UNSEEN is
    (0, 0); slot N - 1 lies 2 cm from slot DUP_LO (the same landmark, mapped twice); slot TIE sits
    on a multiple of 1/8 so that mirror images at 1/16 are at exactly equal distances."""
    side = int(np.ceil(np.sqrt(N)))
    g = np.stack(np.meshgrid(np.arange(side), np.arange(side)), -1).reshape(-1, 2)[:N]
    xy = (g - 0.5 * (side - 1)) * 0.6 + 0.07 + rng.uniform(-0.05, 0.05, (N, 2))
    xy = xy[rng.permutation(N)]
    xy[TIE] = np.round(xy[TIE] * 8.0) / 8.0
    xy[N - 1] = xy[DUP_LO] + [0.01, -0.02]
    xy[UNSEEN] = 0.0
    return xy


def craft_truth(xy, n_map, rng, tie):
    """The truth in the map frame: a shuffled copy of seen slots plus noise (at most 0.05 m per
    coordinate); one landmark for the slot pair DUP_LO, N - 1; none within reach of slot SPUR; two
    mirror images around slot TIE (tie: at exactly equal distances); landmarks near no slot; every
    third entry (k % 3 == 2) with a NaN coordinate, the crafted entries kept off those."""
    N = len(xy)
    noise = lambda: np.clip(rng.normal(size=2) * 0.02, -0.05, 0.05)
    crafted = [xy[DUP_LO] + noise()]
    if n_map >= 5:
        crafted += [xy[TIE] + [0.0625, 0.0], xy[TIE] - [0.0625 if tie else 0.09375, 0.0],
                    np.array([31.0, -29.0])]                      # ... and one missed landmark
    plain = [j for j in rng.permutation(N) if j not in (UNSEEN, DUP_LO, SPUR, TIE, N - 1)]
    fill = [xy[j] + noise() for j in plain]
    far = [np.array([40.0 + 0.7 * (i % 40), 40.0 + 0.7 * (i // 40)]) for i in range(n_map)]
    fill = (fill + far)[:n_map - len(crafted)]
    good = [k for k in rng.permutation(n_map) if k % 3 != 2]
    slots_k = good[:len(crafted)]
    rest = [k for k in range(n_map) if k not in set(slots_k)]
    t = np.zeros((n_map, 2))
    for k, p in zip(slots_k, crafted):
        t[k] = p
    for k, p in zip(rest, fill):
        t[k] = p
    nan_k = np.arange(2, n_map, 3)
    return t, nan_k


def from_map_frame(pts, frame):
    """The map-frame points seen from the truth's frame: compose(frame, point)."""
    return np.array([synth._compose(frame, np.array([0.0, p[0], p[1]]))[1:] for p in pts])


@functools.lru_cache(maxsize=None)
def handle(name):
    """tests/test_gpu_eval.py's driven handle (its filters on different parities), kept for the
    module: each test overwrites the filters with ekf_set_state."""
    return tge.driven(name)


def load(e, n_map, seed, tie, frame):
    """Crafted filters into the handle and their truth (as the caller of ekf_eval_match has it: in
    the truth's frame, NaNs in). Returns (truth_pose [F, 3], truth_lm [F, n_map, 2])."""
    rng = np.random.default_rng(seed)
    pose = np.zeros((e.F, 3))
    lm = np.zeros((e.F, n_map, 2))
    for f in range(e.F):
        x, S = tge.spd_fixture(e.N, rng)
        xy = craft_slots(e.N, rng)
        x[3:] = xy.reshape(-1)
        e.set_state(x, S, counter=e.N, f=f)
        t, nan_k = craft_truth(xy, n_map, rng, tie)
        if frame is not None:
            t = from_map_frame(t, frame)
        t[nan_k, nan_k // 3 % 2] = np.nan
        lm[f] = t
        pose[f] = x[:3] + rng.normal(size=3) * [0.01, 0.05, 0.05]
    return pose, lm


def reference(e, f, truth_lm_f, frame, max_dist, margins):
    x, _, _ = e.state(f, sigma=False)
    xy = x[3:].reshape(e.N, 2)
    tmap = to_map_frame(truth_lm_f, frame)
    match, rec, best, second = match_np(xy, tmap, max_dist, truth_raw=truth_lm_f)
    if margins:      # on the CPU, before anything of the device's is looked at
        s = seen_slots(xy) & np.isfinite(best)
        gate2 = max_dist * max_dist
        assert (np.isinf(second[s]) | (second[s] - best[s] > MARGIN * second[s])).all(), f
        assert (np.abs(best[s] - gate2) > MARGIN * gate2).all(), f
    return match, rec


def same_record(got, want, framed, what):
    """The match record against the restatement: exact. With a frame the counts are exact under
    the margins asserted above, and max_match_dist, a distance to a transformed point, is within
    the transform's own bound: 8 eps (|x| + |y| + |x0| + |y0|) per coordinate on matched
    landmarks within 7 m of the origin, 8 * 2^-52 * 14.75 = 2.6e-14, times sqrt(2) for the two
    coordinates: 4e-14."""
    if not framed:
        assert got.tobytes() == want.tobytes(), (what, got, want)
        return
    for k in ("n_truth", "n_matched", "n_primary", "n_dup", "n_spurious", "n_missed"):
        assert got[k] == want[k], (what, k, got, want)
    d = abs(got["max_match_dist"] - want["max_match_dist"])
    print(f"{what}: max_match_dist {got['max_match_dist']!r}, |d| {d:.3g}")
    assert d <= 4e-14, what


def permuted(truth_lm, match):
    """truth_perm[f, j] = truth_lm[f, match[f, j]], NaN where match < 0: what ekf_eval takes."""
    F, N = match.shape
    out = np.full((F, N, 2), np.nan)
    for f in range(F):
        hit = match[f] >= 0
        out[f, hit] = truth_lm[f, match[f, hit]]
    return out


def n_maps(name):
    N = tge.HANDLES[name][0]
    return [1, 5, N - 1, N + 7] + ([1024] if name == "f32-257" else [])


CASES = [(name, n_map) for name in HANDLES for n_map in n_maps(name)]


# ---- 1: crafted filters --------------------------------------------------------------------------

@pytest.mark.parametrize("name,n_map", CASES, ids=[f"{a}-{b}" for a, b in CASES])
def test_match_and_score_of_crafted_filters(name, n_map):
    pyekf.poison_lds()
    e = handle(name)
    assert e.path == tge.HANDLES[name][3]
    for frame, tie in ((None, True), (FRAME, False)):
        what = f"{name} n_map {n_map} frame {frame is not None}"
        pose, lm = load(e, n_map, 1000 + n_map, tie, frame)
        refs = [reference(e, f, lm[f], frame, MAX_DIST, margins=frame is not None)
                for f in range(e.F)]
        recs, mrecs, match = e.eval_match(pose, lm, MAX_DIST, frame)
        for f in range(e.F):
            want_match, want = refs[f]
            assert (match[f] == want_match).all(), (what, f)
            same_record(mrecs[f], want, frame is not None, (what, f))
            assert match[f, UNSEEN] == -1 and match[f, SPUR] == -1
            assert mrecs[f]["n_matched"] > 0 and mrecs[f]["max_match_dist"] <= MAX_DIST
            # slot 256 of the 257 is lane 0's second slot, and a seen one: the duplicate
            assert match[f, e.N - 1] == match[f, DUP_LO] >= 0
            if n_map >= 5:
                assert mrecs[f]["n_dup"] > 0 and mrecs[f]["n_spurious"] > 0, what
                assert mrecs[f]["n_missed"] > 0, what
                assert match[f, TIE] >= 0
                if tie:     # two truth landmarks at the same distance: the lower index
                    x, _, _ = e.state(f, sigma=False)
                    d2 = sq_distances(x[3:].reshape(e.N, 2), to_map_frame(lm[f], None))[TIE]
                    assert (d2 == d2.min()).sum() == 2
                    assert match[f, TIE] == np.flatnonzero(d2 == d2.min())[0]
            assert recs[f]["n_seen"] == e.N - 1
            assert recs[f]["n_eval"] == mrecs[f]["n_matched"]
        # the record: ekf_eval fed the truth in slot order, byte for byte
        want = e.eval(pose, permuted(lm, match), frame)
        assert recs.tobytes() == want.tobytes(), what
        again = e.eval_match(pose, lm, MAX_DIST, frame)
        assert again[0].tobytes() == recs.tobytes() and again[1].tobytes() == mrecs.tobytes()
        assert again[2].tobytes() == match.tobytes(), what


def test_gate_extremes_on_the_device():
    """max_dist = 0 (only a slot exactly on a truth landmark matches) and +infinity (every seen
    slot matches its nearest truth landmark)."""
    pyekf.poison_lds()
    e = handle("f64-65")
    pose, lm = load(e, e.N + 7, 77, True, None)
    for f in range(e.F):
        x, _, _ = e.state(f, sigma=False)
        lm[f, 0] = x[3 + 2 * 9:5 + 2 * 9]              # truth 0 exactly on slot 9
    for md in (0.0, np.inf):
        recs, mrecs, match = e.eval_match(pose, lm, md)
        for f in range(e.F):
            want_match, want = reference(e, f, lm[f], None, md, margins=False)
            assert (match[f] == want_match).all() and mrecs[f].tobytes() == want.tobytes()
            if md == 0.0:
                assert mrecs[f]["n_matched"] == 1 and match[f, 9] == 0
                assert mrecs[f]["max_match_dist"] == 0.0
            else:
                assert mrecs[f]["n_spurious"] == 0 and mrecs[f]["n_matched"] == e.N - 1
        assert recs.tobytes() == e.eval(pose, permuted(lm, match)).tobytes()


def test_profile_kinds_of_the_scoring_kernels():
    """ekf_profile_read kinds 5 (k_eval) and 6 (k_eval_match): one timed dispatch per call, and the
    events change nothing of the result."""
    pyekf.poison_lds()
    e = handle("f64-65")
    pose, lm = load(e, e.N - 1, 9, True, None)
    plain = e.eval_match(pose, lm, MAX_DIST)
    e.profile(True)
    timed = e.eval_match(pose, lm, MAX_DIST)
    e.eval(pose, permuted(lm, timed[2]))
    e.eval_match(pose, lm, MAX_DIST)
    (n5, ms5), (n6, ms6) = e.profile_read(5), e.profile_read(6)
    e.profile(False)
    assert (n5, n6) == (1, 2) and 0.0 < ms5 < 100.0 and 0.0 < ms6 < 100.0
    assert e.profile_read(6)[0] == 0
    assert all(a.tobytes() == b.tobytes() for a, b in zip(plain, timed))


# ---- 2: argument errors --------------------------------------------------------------------------

def test_argument_errors_touch_nothing():
    pyekf.poison_lds()
    e = handle("resident50")
    L = pyekf.lib()
    pose, lm = load(e, 12, 5, True, None)
    out = np.zeros(e.F, pyekf.EVAL_DTYPE)
    out["n_seen"] = 7
    mrec = np.zeros(e.F, pyekf.MATCH_DTYPE)
    mrec["n_truth"] = 7
    match = np.full((e.F, e.N), 7, np.int32)
    p, t, o, m, k = (a.ctypes.data for a in (pose, lm, out, mrec, match))
    for args in ((None, t, 12, None, MAX_DIST, o, m, k), (p, None, 12, None, MAX_DIST, o, m, k),
                 (p, t, 12, None, MAX_DIST, None, m, k), (p, t, 0, None, MAX_DIST, o, m, k),
                 (p, t, -1, None, MAX_DIST, o, m, k), (p, t, 1025, None, MAX_DIST, o, m, k),
                 (p, t, 12, None, -1e-300, o, m, k), (p, t, 12, None, float("nan"), o, m, k),
                 (p, t, 12, None, -np.inf, o, m, k)):
        assert L.ekf_eval_match(e.h, *args) == pyekf.EKF_E_ARG, args[2:5]
    assert L.ekf_eval_match(None, p, t, 12, None, MAX_DIST, o, m, k) == pyekf.EKF_E_ARG
    assert (out["n_seen"] == 7).all() and (mrec["n_truth"] == 7).all() and (match == 7).all()
    # the two match outputs are nullable; +infinity is a valid gate
    assert L.ekf_eval_match(e.h, p, t, 12, None, np.inf, o, None, None) == pyekf.EKF_OK
    assert (out["n_seen"] == e.N - 1).all() and (mrec["n_truth"] == 7).all()


# ---- 3: the call leaves the filter alone ---------------------------------------------------------

@pytest.mark.parametrize("N", [64, 50], ids=["pipeline64", "resident50"])
def test_eval_match_leaves_the_filter_alone(N):
    """tests/test_gpu_eval.py's twin-handle test with ekf_eval_match in ekf_eval's place: replay A
    (device-planned, one marker with an id out of range), then the first synchronising call:
    ekf_eval_match on one handle, ekf_get_pose on its twin. Everything read afterwards, and after a
    replay B on top, is the same bytes on both."""
    pyekf.poison_lds()
    F, TA, TB, M = 2, 5, 3, tge.M_DRIVE
    cnt, ids, act, rel, od = tge.drive(N, F, TA + TB, M, 47)
    ids = ids.copy()
    assert cnt[1, 0] >= 2
    ids[1, 0, 1] = N + 5
    dev = tge._gpu((cnt, rel, od, ids, act))
    A = tuple(t[:TA].contiguous() for t in dev)
    B = tuple(t[TA:].contiguous() for t in dev)
    rng = np.random.default_rng(23)
    reads = {}
    for how in ("eval_match", "get_pose"):
        e = pyekf.EKF(n_landmarks=N, n_filters=F)
        assert e.path == (pyekf.EKF_PATH_RESIDENT if N == 50 else pyekf.EKF_PATH_PIPELINE)
        e.trace_enable(16)
        e.replay_on_device(A[0], A[1], A[2], ids=A[3], actions=A[4])
        if how == "eval_match":
            pose = rng.normal(size=(F, 3))
            lm = rng.normal(size=(F, N + 9, 2)) * 3.0
            got = e.eval_match(pose, lm, 0.5)
        else:
            e.pose(0)
        mid, status = tge._everything(e, M)
        assert status[0] == pyekf.EKF_FLAG_RANGE and status[1] == 0
        assert [m[5] for m in mid] == [TA] * F
        if how == "eval_match":
            assert (got[0]["n_seen"] > 0).all()
            again = e.eval_match(pose, lm, 0.5)
            assert all(a.tobytes() == b.tobytes() for a, b in zip(got, again))
            assert tge._everything(e, M) == (mid, [0] * F)
        e.replay_on_device(B[0], B[1], B[2], ids=B[3], actions=B[4])
        if how == "eval_match":
            e.eval_match(pose, lm, 0.5)
        reads[how] = (mid, status, tge._everything(e, M))
        e.close()
    assert reads["eval_match"] == reads["get_pose"]


# ---- 4: known ids end in the identity ------------------------------------------------------------

@pytest.mark.parametrize("N,F,seed,start,path",
                         [(50, 4, 20240328, (0.0, 0.0, -1.0), pyekf.EKF_PATH_RESIDENT),
                          (128, 2, 20240336, (0.4, 0.3, -1.2), pyekf.EKF_PATH_PIPELINE)],
                         ids=["resident50", "pipeline128"])
def test_known_ids_end_in_the_identity(N, F, seed, start, path):
    """After a known-id run slot j is landmark j: with a gate below half the smallest landmark
    separation and above the largest landmark error, every seen slot matches its own landmark and
    the record is ekf_sim_eval's."""
    pyekf.poison_lds()
    T = 12
    sw = synth.swarm(N, F, T, seed=seed, survey=False, start_pose=start)
    sep = min(np.sqrt(sq_distances(m, m)[~np.eye(len(m), dtype=bool)].min()) for m in sw.landmarks)
    max_dist = 0.45 * sep
    assert max_dist < 0.5 * sep
    e = pyekf.EKF(n_landmarks=N, n_filters=F)
    assert e.path == path
    sim = pyekf.Sim(e, sw.landmarks, seed=int(sw.seeds[0]), ticks_per_msg=sw.wheel.shape[1],
                    max_markers=min(16, sw.landmarks.shape[1]), marker_stride=sw.ids.shape[2],
                    start_theta=start[0], start_x=start[1], start_y=start[2], record=1)
    sim.run(sw.cmd, sw.sense)
    plain = sim.eval()
    print(f"separation {sep:.4f}, max_dist {max_dist:.4f}, lm_max_err {plain['lm_max_err']}")
    assert (plain["lm_max_err"] < max_dist).all()
    recs, mrecs, match = sim.eval_match(max_dist)
    for f in range(F):
        x, _, _ = e.state(f, sigma=False)
        seen = seen_slots(x[3:].reshape(N, 2))
        assert seen.any() and (match[f, seen] == np.flatnonzero(seen)).all(), f
        assert (match[f, ~seen] == -1).all()
    assert (mrecs["n_dup"] == 0).all() and (mrecs["n_spurious"] == 0).all()
    assert (mrecs["n_truth"] == N).all() and (mrecs["n_matched"] == plain["n_seen"]).all()
    assert recs.tobytes() == plain.tobytes()
    _, truth = sim.poses()
    via = e.eval_match(truth[-1], sw.landmarks, max_dist, frame=start)
    assert via[0].tobytes() == recs.tobytes() and via[1].tobytes() == mrecs.tobytes()
    assert via[2].tobytes() == match.tobytes()
    sim.close()
    e.close()
