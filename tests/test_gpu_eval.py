"""ekf_get_marginals, ekf_eval and ekf_sim_eval (include/ekf.h, include/ekf_sim.h; kernels in
ekf-slam_amd/csrc/ekf_eval.hip) on the GPU.

The reference in every case is ekf_get_state of the same handle, read after the call under test,
plus numpy. What the kernels gather is compared bit for bit. What they compute is restated below
operation for operation in IEEE doubles (the kernels are built with -ffp-contract=off), so every
per-landmark term has the same bits on both sides and only the order of a sum differs:
  pose_err (no frame), pose_cov, lm_max_err, the counts and the flags    exact
  pose_nees    |d| <= 32 k(P) eps NEES against an extended-precision reference, k = numpy's cond(P)
  the sums     |d| <= N eps sum|terms|
(eps = 2^-52; tests/test_eval_math_host.py has the reasoning and the arithmetic's own tests.)"""
import functools

import numpy as np
import pytest

import pyekf
from pyekf import synth

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -52
LD = np.longdouble
POSE_NOT_PD, LM_NOT_PD = pyekf.EKF_EVAL_POSE_NOT_PD, pyekf.EKF_EVAL_LM_NOT_PD


# ---- the numpy restatement -----------------------------------------------------------------------

def wrap(a):
    d = np.fmod(np.float64(a) + np.pi, 2.0 * np.pi)
    return d + np.pi if d <= 0.0 else d - np.pi


def _ok(d):
    return bool(d > 0.0 and np.isfinite(d))


def nees3(P, e):
    """eval_math.hpp nees3, operation for operation; P = (tt tx ty xx xy yy). None: not PD."""
    with np.errstate(all="ignore"):
        d0 = P[0]
        if not _ok(d0):
            return None
        l10, l20 = P[1] / d0, P[2] / d0
        d1 = P[3] - l10 * P[1]
        if not _ok(d1):
            return None
        u21 = P[4] - l20 * P[1]
        l21 = u21 / d1
        d2 = P[5] - l20 * P[2] - l21 * u21
        if not _ok(d2):
            return None
        z0 = e[0]
        z1 = e[1] - l10 * z0
        z2 = e[2] - l20 * z0 - l21 * z1
        return z0 * z0 / d0 + z1 * z1 / d1 + z2 * z2 / d2


def nees2(C, e0, e1):
    with np.errstate(all="ignore"):
        d0 = C[0]
        if not _ok(d0):
            return None
        l = C[1] / d0
        d1 = C[2] - l * C[1]
        if not _ok(d1):
            return None
        z1 = e1 - l * e0
        return e0 * e0 / d0 + z1 * z1 / d1


def nees3_ld(P, e):
    """The same in extended precision, by the adjugate (the reference of the k(P) bound)."""
    M = np.array([[P[0], P[1], P[2]], [P[1], P[3], P[4]], [P[2], P[4], P[5]]], LD)
    e = np.asarray(e, LD)
    adj = np.empty((3, 3), LD)
    for i in range(3):
        for j in range(3):
            r = [k for k in range(3) if k != j]
            c = [k for k in range(3) if k != i]
            m = M[np.ix_(r, c)]
            adj[i, j] = (-1) ** (i + j) * (m[0, 0] * m[1, 1] - m[0, 1] * m[1, 0])
    det = sum(M[0, j] * adj[j, 0] for j in range(3))
    return e @ adj @ e / det


def marginals_np(x, S, N):
    pose = x[:3].copy()
    cov = 0.5 * (S[:3, :3] + S[:3, :3].T)
    r = 3 + 2 * np.arange(N)
    lm = np.zeros(N, pyekf.LM_MARGINAL_DTYPE)
    lm["xy"] = np.stack([x[r], x[r + 1]], 1)
    lm["cov"] = np.stack([S[r, r], 0.5 * (S[r, r + 1] + S[r + 1, r]), S[r + 1, r + 1]], 1)
    lm["seen"] = ~((x[r] == 0.0) & (x[r + 1] == 0.0))
    return pose, cov, lm


def score_np(x, S, N, truth_pose, truth_lm, n_map):
    """One filter's record, frame = NULL: the exact fields, the NEES reference with its bound,
    and each sum's terms."""
    pose, cov, lm = marginals_np(x, S, N)
    P = np.array([cov[0, 0], cov[0, 1], cov[0, 2], cov[1, 1], cov[1, 2], cov[2, 2]])
    err = np.array([wrap(pose[0] - truth_pose[0]), pose[1] - truth_pose[1],
                    pose[2] - truth_pose[2]])
    out = {"pose_err": err, "pose_cov": P, "flags": 0}
    q = nees3(P, err)
    if q is None:
        out["flags"] |= POSE_NOT_PD
        out["pose_nees"] = None
    else:
        M = np.array([[P[0], P[1], P[2]], [P[1], P[3], P[4]], [P[2], P[4], P[5]]])
        ref = nees3_ld(P, err)
        out["pose_nees"] = (ref, 32 * np.linalg.cond(M) * EPS * ref)
    sq, nees, tr, n_seen, n_eval = [], [], [], 0, 0
    for j in range(N):
        if not lm["seen"][j]:
            continue
        n_seen += 1
        C = lm["cov"][j]
        tr.append(C[0] + C[2])
        if j >= n_map or np.isnan(truth_lm[j]).any():
            continue
        dx, dy = lm["xy"][j, 0] - truth_lm[j, 0], lm["xy"][j, 1] - truth_lm[j, 1]
        n_eval += 1
        sq.append(dx * dx + dy * dy)
        q = nees2(C, dx, dy)
        if q is None:
            out["flags"] |= LM_NOT_PD
        else:
            nees.append(q)
    out.update(n_seen=n_seen, n_eval=n_eval, n_nees=len(nees), lm_sq_err=sq, lm_nees=nees,
               lm_var_trace=tr, lm_max_err=float(np.sqrt(max(sq))) if sq else 0.0)
    return out


def check_record(rec, ref, N, what):
    assert rec["pose_err"].tobytes() == ref["pose_err"].tobytes(), what
    assert rec["pose_cov"].tobytes() == ref["pose_cov"].tobytes(), what
    for k in ("n_seen", "n_eval", "n_nees", "flags"):
        assert int(rec[k]) == ref[k], (what, k, int(rec[k]), ref[k])
    if ref["pose_nees"] is None:
        assert np.isnan(rec["pose_nees"]), what
    else:
        want, bound = ref["pose_nees"]
        d = abs(LD(rec["pose_nees"]) - want)
        print(f"{what}: pose NEES {rec['pose_nees']:.6g}, |d| {float(d):.3g}, "
              f"bound {float(bound):.3g}")
        assert d <= bound, what
    for k in ("lm_sq_err", "lm_nees", "lm_var_trace"):
        terms = np.asarray(ref[k], LD)
        want, mag = terms.sum(), np.abs(terms).sum()
        d = abs(LD(rec[k]) - want)
        print(f"{what}: {k} {rec[k]:.6g}, |d| {float(d):.3g}, bound {float(N * EPS * mag):.3g}")
        assert d <= N * EPS * mag, (what, k)
    assert rec["lm_max_err"] == ref["lm_max_err"], what


def check_eval(e, truth_pose, truth_lm, n_map, what, frame=None):
    """ekf_eval twice (the same bytes), then the state read back and scored by numpy."""
    tl = None if n_map == 0 else truth_lm[:, :n_map]
    recs = e.eval(truth_pose, tl, frame)
    again = e.eval(truth_pose, tl, frame)
    assert recs.tobytes() == again.tobytes(), what
    for f in range(e.F):
        x, S, _ = e.state(f)
        check_record(recs[f], score_np(x, S, e.N, truth_pose[f], truth_lm[f], n_map),
                     e.N, f"{what} filter {f}")
    return recs


# ---- handles and drives --------------------------------------------------------------------------

HANDLES = {  # N, F, dtype, path
    "resident50": (50, 3, pyekf.EKF_F64, pyekf.EKF_PATH_RESIDENT),
    "f64-64": (64, 2, pyekf.EKF_F64, pyekf.EKF_PATH_PIPELINE),
    "f64-65": (65, 2, pyekf.EKF_F64, pyekf.EKF_PATH_PIPELINE),
    "f32-257": (257, 2, pyekf.EKF_F32, pyekf.EKF_PATH_PIPELINE),
    "f64-257": (257, 2, pyekf.EKF_F64, pyekf.EKF_PATH_PIPELINE),
}
T_DRIVE, M_DRIVE = 5, 6


@functools.lru_cache(maxsize=None)
def drive(N, F, T=T_DRIVE + 1, M=M_DRIVE, seed=31):
    """F robots x T messages of at most M markers with known ids (robot f: synth.synthetic seed +
    f); the landmark of each robot's first marker is relabelled to slot N - 1, so that the last
    slot (one past a 256-thread stride at N = 257) is a seen one."""
    cnt = np.zeros((T, F), np.int32)
    ids = np.zeros((T, F, M), np.int32)
    act = np.zeros((T, F, M), np.int32)
    rel = np.zeros((T, F, M, 2))
    od = np.zeros((T, F, 3))
    for f in range(F):
        sc = synth.synthetic(N, T, seed=seed + f, max_markers=M)
        i = np.maximum(sc.ids, 0)
        a = int(i[0, 0])
        i = np.where(i == a, N - 1, np.where(i == N - 1, a, i))
        cnt[:, f], ids[:, f], act[:, f], rel[:, f] = sc.count, i, sc.actions, sc.rel
        od[:, f] = pyekf.odometry(sc)
    assert (cnt > 0).all()
    return cnt, ids, act, rel, od


def driven(name):
    """The handle after T_DRIVE messages to every filter and one more to filter 1 alone, so that
    the filters of one handle are on different parities."""
    N, F, dtype, path = HANDLES[name]
    e = pyekf.EKF(n_landmarks=N, n_filters=F, dtype=dtype)
    assert e.path == path
    cnt, ids, act, rel, od = drive(N, F)
    e.replay(cnt[:T_DRIVE], rel[:T_DRIVE], od[:T_DRIVE], ids=ids[:T_DRIVE], actions=act[:T_DRIVE])
    one = cnt[T_DRIVE:].copy()
    one[:, np.arange(F) != 1] = 0
    e.replay(one, rel[T_DRIVE:], od[T_DRIVE:], ids=ids[T_DRIVE:], actions=act[T_DRIVE:])
    return e


def truth_near(e, rng, nan_every=3):
    """Truth drawn near the estimate: every slot gets one (an unseen slot's must be ignored), but
    every nan_every-th seen slot, the first one included, has a NaN coordinate. Also returns each
    filter's seen slots."""
    pose = np.zeros((e.F, 3))
    lm = np.zeros((e.F, e.N, 2))
    seen = []
    for f in range(e.F):
        x, _, _ = e.state(f, sigma=False)
        pose[f] = x[:3] + rng.normal(size=3) * [0.01, 0.05, 0.05]
        xy = x[3:].reshape(e.N, 2)
        lm[f] = xy + rng.normal(size=(e.N, 2)) * 0.05
        seen.append(np.flatnonzero((xy != 0.0).any(1)))
        lm[f, seen[f][::nan_every], np.arange(len(seen[f][::nan_every])) % 2] = np.nan
    return pose, lm, seen


# ---- 1: marginals --------------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(HANDLES))
def test_marginals_equal_get_state_bit_for_bit(name):
    e = driven(name)
    each = [e.marginals(f) for f in range(e.F)]
    pose_all, cov_all, lm_all, cnt_all = e.marginals()
    seen_last = 0
    for f in range(e.F):
        x, S, c = e.state(f)
        pose, cov, lm = marginals_np(x, S, e.N)
        gp, gc, gl, gcnt = each[f]
        assert gp.tobytes() == pose.tobytes() and gc.tobytes() == cov.tobytes(), f
        assert gl.tobytes() == lm.tobytes(), f      # xy, the blocks, seen and the zero pad
        assert gcnt == c, f
        assert pose_all[f].tobytes() == gp.tobytes() and cov_all[f].tobytes() == gc.tobytes()
        assert lm_all[f].tobytes() == gl.tobytes() and cnt_all[f] == c
        assert 0 < lm["seen"].sum() < e.N
        seen_last += int(lm["seen"][e.N - 1])
    assert seen_last == e.F   # the last slot is a seen one in every filter
    # every output is nullable
    L = pyekf.lib()
    assert L.ekf_get_marginals(e.h, 0, None, None, None, None) == pyekf.EKF_OK
    c = np.zeros(1, np.uint32)
    assert L.ekf_get_marginals(e.h, 1, None, None, None, c.ctypes.data) == pyekf.EKF_OK
    assert c[0] == each[1][3]
    assert L.ekf_get_marginals(e.h, e.F, None, None, None, None) == pyekf.EKF_E_ARG
    e.close()


# ---- 2: ekf_eval against numpy on the read-back state --------------------------------------------

@pytest.mark.parametrize("name", list(HANDLES))
def test_eval_against_numpy(name):
    e = driven(name)
    rng = np.random.default_rng(sum(map(ord, name)))
    pose, lm, seen = truth_near(e, rng)
    assert all(len(s) >= 3 and s[-1] == e.N - 1 for s in seen)
    # one case with n_map < N: every filter keeps its second seen slot (the first has no truth)
    # and loses at least its last
    n_map = max(int(s[1]) for s in seen) + 1 if name == "f64-65" else e.N
    assert n_map < e.N or name != "f64-65"
    recs = check_eval(e, pose, lm, n_map, name)
    assert (recs["n_eval"] > 0).all() and (recs["n_eval"] < recs["n_seen"]).all()
    assert (recs["n_nees"] == recs["n_eval"]).all() and (recs["flags"] == 0).all()
    # poses only
    recs0 = check_eval(e, pose, lm, 0, name + " poses only")
    assert (recs0["n_eval"] == 0).all() and (recs0["n_seen"] == recs["n_seen"]).all()
    assert recs0["pose_nees"].tobytes() == recs["pose_nees"].tobytes()
    # argument checks: nothing is touched
    L = pyekf.lib()
    out = np.zeros(e.F, pyekf.EVAL_DTYPE)
    out["n_seen"] = 7
    tl = np.ascontiguousarray(lm)
    for args in ((None, tl.ctypes.data, e.N, None, out.ctypes.data),
                 (pose.ctypes.data, tl.ctypes.data, e.N, None, None),
                 (pose.ctypes.data, tl.ctypes.data, e.N + 1, None, out.ctypes.data),
                 (pose.ctypes.data, tl.ctypes.data, -1, None, out.ctypes.data),
                 (pose.ctypes.data, None, 1, None, out.ctypes.data)):
        assert L.ekf_eval(e.h, *args) == pyekf.EKF_E_ARG
    assert (out["n_seen"] == 7).all()
    e.close()


# ---- 3: a fresh handle ---------------------------------------------------------------------------

@pytest.mark.parametrize("N,dtype", [(50, pyekf.EKF_F64), (257, pyekf.EKF_F32)])
def test_fresh_handle(N, dtype):
    e = pyekf.EKF(n_landmarks=N, n_filters=2, dtype=dtype)
    rng = np.random.default_rng(3)
    recs = e.eval(rng.normal(size=(2, 3)) * 0.1, rng.normal(size=(2, N, 2)))
    for r in recs:
        assert r["flags"] == POSE_NOT_PD and np.isnan(r["pose_nees"])
        assert r["n_seen"] == 0 and r["n_eval"] == 0 and r["n_nees"] == 0
        for k in ("pose_err", "pose_cov", "lm_sq_err", "lm_nees", "lm_max_err", "lm_var_trace"):
            assert np.isfinite(r[k]).all(), k
        assert (r["pose_cov"] == 0).all() and r["lm_var_trace"] == 0.0
    pose, cov, lm, cnt = e.marginals()
    assert (lm["seen"] == 0).all() and (lm["cov"][..., 0] == e.cfg.init_var).all()
    assert (cnt == 0).all() and (cov == 0).all()
    s = pyekf.eval_summary(recs)
    assert s["n_pose_nees"] == 0 and np.isnan(s["anees_pose"]) and np.isnan(s["lm_rmse"])
    e.close()


# ---- 4: ekf_set_state fixtures -------------------------------------------------------------------

def spd_fixture(N, rng):
    n = 3 + 2 * N
    A = rng.normal(size=(n, n)) / np.sqrt(n)
    S = A @ A.T * 0.02 + np.diag(rng.uniform(0.05, 0.2, n))
    x = rng.normal(size=n)
    x[3 + 2 * 7:3 + 2 * 7 + 2] = 0.0      # slot 7 unseen
    return x, 0.5 * (S + S.T)


@pytest.mark.parametrize("dtype", [pyekf.EKF_F32, pyekf.EKF_F64], ids=["f32", "resident"])
def test_a_sigma_that_is_not_symmetric_scores_as_its_symmetric_part(dtype):
    N = 50
    e = pyekf.EKF(n_landmarks=N, n_filters=2, dtype=dtype)
    assert e.path == (pyekf.EKF_PATH_RESIDENT if dtype == pyekf.EKF_F64 else
                      pyekf.EKF_PATH_PIPELINE)
    rng = np.random.default_rng(17)
    for f in range(2):
        x, S = spd_fixture(N, rng)
        K = rng.normal(size=S.shape) * 1e-3
        e.set_state(x, S + (K - K.T), counter=N, f=f)
        _, back, _ = e.state(f)
        assert (back != back.T).any()          # stored as given
    pose, lm, _ = truth_near(e, rng, nan_every=5)
    recs = check_eval(e, pose, lm, N, "not symmetric")
    assert (recs["flags"] == 0).all() and (recs["n_seen"] == N - 1).all()
    assert (recs["n_nees"] == recs["n_eval"]).all() and (recs["n_eval"] > 30).all()
    assert np.isfinite(recs["pose_nees"]).all()
    for f in range(2):                          # the marginals come back symmetrised
        _, cov, _, _ = e.marginals(f)
        assert (cov == cov.T).all()
    e.close()


def test_a_landmark_block_that_is_not_positive_definite():
    N, bad = 64, 21
    e = pyekf.EKF(n_landmarks=N, n_filters=1)
    assert e.path == pyekf.EKF_PATH_PIPELINE
    rng = np.random.default_rng(18)
    x, S = spd_fixture(N, rng)
    r = 3 + 2 * bad
    S[r:r + 2, r:r + 2] = [[0.1, 0.2], [0.2, 0.1]]
    e.set_state(x, S, counter=N)
    pose, lm, _ = truth_near(e, rng, nan_every=N + 1)   # slot 0 alone has no truth
    assert not np.isnan(lm[0, bad]).any()
    recs = check_eval(e, pose, lm, N, "not positive definite")
    assert recs["flags"][0] == LM_NOT_PD
    assert recs["n_seen"][0] == N - 1 and recs["n_eval"][0] == N - 2
    assert recs["n_nees"][0] == recs["n_eval"][0] - 1
    e.close()


# ---- 5: the call leaves the filter alone ---------------------------------------------------------

def _gpu(arrs):
    import torch
    return tuple(torch.from_numpy(np.array(a, order="C")).cuda() for a in arrs)


def _everything(e, m):
    """State, Sigma, counter, decisions, trace count and, last (reading clears them), the status
    flags of every filter."""
    out = []
    for f in range(e.F):
        x, S, c = e.state(f)
        j, nw = e.decisions(m, f)
        out.append((x.tobytes(), S.tobytes(), c, j.tobytes(), nw.tobytes(), e.trace_count(f),
                    e.map_odom(f).tobytes()))
    return out, [e.status(f) for f in range(e.F)]


@pytest.mark.parametrize("N,resident_env", [(64, None), (50, None), (50, "0")],
                         ids=["pipeline64", "resident50", "resident50-forced-to-pipeline"])
def test_eval_leaves_the_filter_alone(N, resident_env, monkeypatch):
    """Replay A (device-planned, odd T, one marker with an id out of range), then the first
    synchronising call: ekf_eval on one handle, ekf_get_pose on its twin. Everything read
    afterwards, and after a replay B on top, is the same bytes on both."""
    if resident_env is not None:
        monkeypatch.setenv("EKF_RESIDENT", resident_env)
    F, TA, TB = 2, 5, 3
    cnt, ids, act, rel, od = drive(N, F, TA + TB, M_DRIVE, 47)
    ids = ids.copy()
    assert cnt[1, 0] >= 2
    ids[1, 0, 1] = N + 5          # skipped on the device: EKF_FLAG_RANGE in filter 0's status
    dev = _gpu((cnt, rel, od, ids, act))
    A = tuple(t[:TA].contiguous() for t in dev)
    B = tuple(t[TA:].contiguous() for t in dev)
    rng = np.random.default_rng(19)
    reads = {}
    for how in ("eval", "get_pose"):
        e = pyekf.EKF(n_landmarks=N, n_filters=F)
        assert e.path == (pyekf.EKF_PATH_RESIDENT if N == 50 and resident_env is None else
                          pyekf.EKF_PATH_PIPELINE)
        e.trace_enable(16)
        e.replay_on_device(A[0], A[1], A[2], ids=A[3], actions=A[4])
        # nothing has synchronised: the planning state of replay A is still on the device
        if how == "eval":
            pose = rng.normal(size=(F, 3))
            lm = rng.normal(size=(F, N, 2))
            recs = e.eval(pose, lm)
        else:
            e.pose(0)
        mid, status = _everything(e, M_DRIVE)
        assert status[0] == pyekf.EKF_FLAG_RANGE and status[1] == 0
        assert [m[5] for m in mid] == [TA] * F          # one trace record per message, no more
        if how == "eval":
            for f in range(F):
                x, S, _ = e.state(f)
                check_record(recs[f], score_np(x, S, N, pose[f], lm[f], N), N,
                             f"after the device replay, filter {f}")
            assert (recs["n_seen"] > 0).all()
            again = e.eval(pose, lm)
            assert again.tobytes() == recs.tobytes()
            assert _everything(e, M_DRIVE) == (mid, [0] * F)   # (the read above cleared the flags)
        e.replay_on_device(B[0], B[1], B[2], ids=B[3], actions=B[4])
        if how == "eval":
            e.eval(pose, lm)
        reads[how] = (mid, status, _everything(e, M_DRIVE))
        e.close()
    assert reads["eval"] == reads["get_pose"]


# ---- 6: ekf_sim_eval -----------------------------------------------------------------------------

@pytest.mark.parametrize("N,F,start,path",
                         [(50, 8, (0.0, 0.0, -1.0), pyekf.EKF_PATH_RESIDENT),
                          (128, 4, (0.4, 0.3, -1.2), pyekf.EKF_PATH_PIPELINE)],
                         ids=["resident50", "pipeline128"])
def test_sim_eval_equals_eval_fed_the_simulators_truth(N, F, start, path):
    T = 12
    sw = synth.swarm(N, F, T, survey=False, start_pose=start)
    e = pyekf.EKF(n_landmarks=N, n_filters=F)
    assert e.path == path
    sim = pyekf.Sim(e, sw.landmarks, seed=int(sw.seeds[0]), ticks_per_msg=sw.wheel.shape[1],
                    max_markers=min(16, sw.landmarks.shape[1]), marker_stride=sw.ids.shape[2],
                    start_theta=start[0], start_x=start[1], start_y=start[2], record=1)
    sim.run(sw.cmd, sw.sense)
    recs = sim.eval()
    _, truth = sim.poses()
    assert truth.shape == (T, F, 3)
    want = e.eval(truth[-1], sw.landmarks, frame=start)
    assert recs.tobytes() == want.tobytes()
    assert sim.eval().tobytes() == recs.tobytes()
    assert (recs["n_seen"] > 0).all() and (recs["n_eval"] == recs["n_seen"]).all()
    assert (recs["flags"] == 0).all()
    # the frame on the device against its numpy restatement (synth's compose / inverse are
    # geom.hpp's): the device's sin and cos are within an ulp of numpy's, on coordinates of a few
    # metres
    inv = synth._inverse(start)
    for f in range(F):
        t = synth._compose(inv, truth[-1, f])
        x = e.pose(f)
        ref = np.array([wrap(x[0] - wrap(t[0])), x[1] - t[1], x[2] - t[2]])
        assert np.abs(recs["pose_err"][f] - ref).max() < 1e-13, f
    s = pyekf.eval_summary(recs)
    print("summary:", s)
    assert all(np.isfinite(v) for v in s.values())
    assert s["n"] == F and s["n_pose_nees"] == F
    sim.close()
    e.close()
