"""ekf_copy_state on the GPU against the host route it replaces.

The expected state of a destination filter is never taken from the code under test: a twin handle
is filled by ekf_get_state + ekf_get_map_odom on the source and ekf_set_state + ekf_set_odom on the
twin (for a grown map padded here with state 0, the destination's init_var on the new diagonal and
0 elsewhere), and the device-copied handle must equal it bit for bit, right after the copy and again
after three further messages on both (the first of them without ekf_set_odom, so it predicts from
the carried t_odom_robot; together they cover the parity, what the destination forgets and the
zeroed padding, which the Σ pass reads).

Map sizes N = 14, 15, 30, 31, 62, 63 (n = 31, 33, 63, 65, 127, 129) sit on either side of the
kernel's 64-wide tile edge, of the row padding (16 fp64 / 32 fp32 elements) and of the resident
limit n <= 128. The source is populated by five known-id messages (an odd number: source and
destination then stand on different Σ copies) at a prior of 100, which fp32 holds from message 0.
"""
import functools

import numpy as np
import pytest

import pyekf
from pyekf import synth

pytestmark = pytest.mark.gpu

T1, T2 = 5, 3
SRC_VAR, DST_VAR = 100.0, 64.0  # (different: a grown map takes the destination's)
KINDS = ("res", "p64", "p32")
SIZES = [(14, 14), (15, 15), (31, 31), (62, 62), (63, 63), (30, 31), (31, 63), (62, 63), (14, 30)]


def _resident_fits(N):
    return 3 + 2 * N <= 128


PAIRS = [(ks, kd, ns, nd) for ks in KINDS for kd in KINDS for ns, nd in SIZES
         if (ks != "res" or _resident_fits(ns)) and (kd != "res" or _resident_fits(nd))]


@functools.lru_cache(maxsize=None)
def _messages(N, F):
    """T1 + T2 known-id messages for F filters over a map of N landmarks: ekf_replay's arrays."""
    sw = synth.swarm(N, F, T1 + T2, survey=False, max_markers=14)
    odom = np.repeat(pyekf.odometry(sw.scenario(0))[:, None], F, 1)
    i32 = [np.ascontiguousarray(a, np.int32) for a in (sw.count, sw.ids, sw.actions)]
    return i32[0], i32[1], i32[2], np.ascontiguousarray(sw.rel), np.ascontiguousarray(odom)


def _handle(monkeypatch, kind, N, F=1, var=SRC_VAR):
    """(the path is read from the environment at ekf_create)"""
    if kind == "p64":
        monkeypatch.setenv("EKF_RESIDENT", "0")
    else:
        monkeypatch.delenv("EKF_RESIDENT", raising=False)
    h = pyekf.EKF(N, F, pyekf.EKF_F32 if kind == "p32" else pyekf.EKF_F64, init_var=var)
    assert h.path == (pyekf.EKF_PATH_RESIDENT if kind == "res" else pyekf.EKF_PATH_PIPELINE)
    return h


def _populate(h, N, sl=slice(0, T1)):
    cnt, ids, act, rel, odom = (a[sl] for a in _messages(N, h.F))
    h.replay(cnt, rel, odom, ids=ids, actions=act)
    return odom[-1]  # the handle's t_odom_robot afterwards, [F, 3]


def _snap(h, filters=None):
    """x, the full Σ, the counter and t_map_odom of every filter asked for."""
    out = []
    for f in range(h.F) if filters is None else filters:
        x, S, cnt = h.state(f)
        out.append((x, S, cnt, h.map_odom(f)))
    return out


def _same(a, b, what=""):
    assert len(a) == len(b)
    for k, ((xa, Sa, ca, ta), (xb, Sb, cb, tb)) in enumerate(zip(a, b)):
        np.testing.assert_array_equal(xa, xb, err_msg=f"{what} x of filter {k}")
        np.testing.assert_array_equal(Sa, Sb, err_msg=f"{what} sigma of filter {k}")
        np.testing.assert_array_equal(ta, tb, err_msg=f"{what} tmo of filter {k}")
        assert ca == cb, (what, k)


def _host_route(dst, fd, src, fs, src_odom):
    """The four calls ekf_copy_state is defined by, x and Σ padded for a larger destination."""
    x, S, cnt = src.state(fs)
    tmo = src.map_odom(fs)
    n, nd = src.n, dst.n
    x2, S2 = np.zeros(nd), np.zeros((nd, nd))
    x2[:n] = x
    S2[:n, :n] = S
    S2[np.arange(n, nd), np.arange(n, nd)] = dst.cfg.init_var
    dst.set_state(x2, S2, tmo=tmo, counter=cnt, f=fd)
    assert dst.set_odom(src_odom, fd) == 0


def _continue(h, N, filters):
    """T2 further messages per filter: the first predicts from the handle's own t_odom_robot."""
    cnt, ids, act, rel, odom = _messages(N, h.F)
    for t in range(T1, T1 + T2):
        for f in filters:
            c = int(cnt[t, f])
            if t > T1:
                assert h.set_odom(odom[t, f], f) == 0
            assert h.fake_sensor(ids[t, f, :c], act[t, f, :c], rel[t, f, :c], f) == 0


def _close(*hs):
    for h in hs:
        h.close()


@pytest.mark.parametrize("ks,kd,ns,nd", PAIRS, ids=[f"{a}-{b}-{c}to{d}" for a, b, c, d in PAIRS])
def test_one_filter_equals_the_host_route(monkeypatch, ks, kd, ns, nd):
    src = _handle(monkeypatch, ks, ns)
    odom = _populate(src, ns)
    dst, twin = (_handle(monkeypatch, kd, nd, var=DST_VAR) for _ in range(2))
    before = _snap(src)
    dst.copy_state_from(src, 0, 0)
    _host_route(twin, 0, src, 0, odom[0])
    _same(_snap(dst), _snap(twin), "after the copy:")
    _same(_snap(src), before, "the source:")
    _continue(dst, ns, [0])
    _continue(twin, ns, [0])
    _same(_snap(dst), _snap(twin), "three messages on:")
    assert dst.status() == twin.status() == 0
    _close(src, dst, twin)


@pytest.mark.parametrize("ks,kd,ns,nd", [("res", "p64", 31, 63), ("p32", "p64", 30, 31),
                                         ("p64", "p32", 63, 63), ("p64", "res", 14, 15)])
def test_fork_into_three(monkeypatch, ks, kd, ns, nd):
    """dst_filter < 0 from source filter 2 of three: every destination filter gets its state."""
    src = _handle(monkeypatch, ks, ns, F=3)
    odom = _populate(src, ns)
    dst, twin = (_handle(monkeypatch, kd, nd, F=3, var=DST_VAR) for _ in range(2))
    dst.copy_state_from(src, 2)
    for f in range(3):
        _host_route(twin, f, src, 2, odom[2])
    _same(_snap(dst), _snap(twin), "after the fork:")
    _continue(dst, ns, [0, 1, 2])
    _continue(twin, ns, [0, 1, 2])
    _same(_snap(dst), _snap(twin), "three messages on:")
    _close(src, dst, twin)


@pytest.mark.parametrize("ks,kd,ns,nd", [("p64", "p32", 31, 31), ("res", "p32", 62, 63),
                                         ("p32", "p64", 15, 15)])
def test_swarm_hand_over(monkeypatch, ks, kd, ns, nd):
    """Both < 0: filter f receives filter f (fp64 -> fp32, the survey hand-over, and back)."""
    src = _handle(monkeypatch, ks, ns, F=3)
    odom = _populate(src, ns)
    dst, twin = (_handle(monkeypatch, kd, nd, F=3, var=DST_VAR) for _ in range(2))
    dst.copy_state_from(src)
    for f in range(3):
        _host_route(twin, f, src, f, odom[f])
    _same(_snap(dst), _snap(twin), "after the hand-over:")
    _continue(dst, ns, [0, 1, 2])
    _continue(twin, ns, [0, 1, 2])
    _same(_snap(dst), _snap(twin), "three messages on:")
    _close(src, dst, twin)


@pytest.mark.parametrize("kind,N", [("res", 31), ("p64", 31), ("p32", 63)])
def test_fork_inside_one_handle(monkeypatch, kind, N):
    """dst == src: filters 0 and 2 become filter 1, whose own bytes stay; and a swarm hand-over
    of a handle onto itself touches nothing."""
    h, twin = (_handle(monkeypatch, kind, N, F=3) for _ in range(2))
    odom = _populate(h, N)
    _populate(twin, N)
    # filter 1 one message ahead of the others: its Σ copy is the other one
    cnt, ids, act, rel, od = _messages(N, 3)
    c = int(cnt[T1, 1])
    for e in (h, twin):
        assert e.set_odom(od[T1, 1], 1) == 0
        assert e.fake_sensor(ids[T1, 1, :c], act[T1, 1, :c], rel[T1, 1, :c], 1) == 0
    own = _snap(h, [1])
    for f in (0, 2):
        _host_route(twin, f, twin, 1, od[T1, 1])
    h.copy_state_from(h, 1)
    _same(_snap(h, [1]), own, "the source filter:")
    _same(_snap(h), _snap(twin), "after the fork:")
    h.copy_state_from(h)
    assert pyekf.lib().ekf_copy_state(h.h, 2, h.h, 2) == pyekf.EKF_OK
    _same(_snap(h), _snap(twin), "onto itself:")
    for e in (h, twin):
        for f in range(3):
            c = int(cnt[T1 + 1, f])
            assert e.fake_sensor(ids[T1 + 1, f, :c], act[T1 + 1, f, :c], rel[T1 + 1, f, :c], f) == 0
    _same(_snap(h), _snap(twin), "a message on:")
    _close(h, twin)


@pytest.mark.parametrize("kd", KINDS)
def test_one_to_one_leaves_the_other_filters(monkeypatch, kd):
    """Into filter 1 of three: filters 0 and 2 keep x, Σ, t_map_odom, counter and status."""
    N = 31
    src = _handle(monkeypatch, "p64", N, F=3)
    odom = _populate(src, N)
    dst, twin = (_handle(monkeypatch, kd, N, F=3, var=DST_VAR) for _ in range(2))
    for e in (dst, twin):
        _populate(e, N, slice(0, 2))
    dst.copy_state_from(src, 2, 1)
    _host_route(twin, 1, src, 2, odom[2])
    _same(_snap(dst), _snap(twin))
    assert [dst.status(f) for f in range(3)] == [twin.status(f) for f in range(3)]
    _close(src, dst, twin)


@pytest.mark.parametrize("kind,N", [("p64", 31), ("p32", 31), ("res", 31), ("p64", 63)])
def test_copy_right_after_a_device_replay(monkeypatch, kind, N):
    """The source's planning state is still on the device (ekf_replay_device /
    ekf_replay_resident, no synchronising call since): the copy adopts it, and gives what it gives
    after an ekf_sync — the Σ copy each filter stands on and t_odom_robot included."""
    import torch
    arrs = [torch.from_numpy(np.ascontiguousarray(a[:T1])).cuda() for a in _messages(N, 3)]
    cnt, ids, act, rel, odom = arrs
    out = []
    for synced in (False, True):
        src = _handle(monkeypatch, kind, N, F=3)
        dst = _handle(monkeypatch, "p64", N, F=3, var=DST_VAR)
        src.replay_on_device(cnt, rel, odom, ids=ids, actions=act)
        if synced:
            src.sync()
        dst.copy_state_from(src)
        first = _snap(dst)
        _continue(dst, N, [0, 1, 2])
        out.append((first, _snap(dst)))
        if synced:  # ... which is the host route's
            twin = _handle(monkeypatch, "p64", N, F=3, var=DST_VAR)
            for f in range(3):
                _host_route(twin, f, src, f, _messages(N, 3)[4][T1 - 1, f])
            _same(first, _snap(twin), "against the host route:")
            twin.close()
        _close(src, dst)
    _same(out[0][0], out[1][0], "after the copy:")
    _same(out[0][1], out[1][1], "three messages on:")


@pytest.mark.parametrize("ks,kd", [("p64", "p64"), ("res", "p32"), ("p32", "res")])
def test_pending_predict_is_carried(monkeypatch, ks, kd):
    N = 15
    src = _handle(monkeypatch, ks, N)
    odom = _populate(src, N)
    dst, twin = (_handle(monkeypatch, kd, N, var=DST_VAR) for _ in range(2))
    src.predict()
    dst.copy_state_from(src, 0, 0)
    _host_route(twin, 0, src, 0, odom[0])
    twin.predict()
    cnt, ids, act, rel, _ = _messages(N, 1)
    for e in (dst, twin):
        e.correct(int(ids[T1, 0, 0]), *rel[T1, 0, 0])
    _same(_snap(dst), _snap(twin))
    # and the predict did happen: without it the covariance differs
    plain = _handle(monkeypatch, kd, N, var=DST_VAR)
    _host_route(plain, 0, src, 0, odom[0])
    plain.correct(int(ids[T1, 0, 0]), *rel[T1, 0, 0])
    assert not np.array_equal(plain.state()[1], dst.state()[1])
    _close(src, dst, twin, plain)


@pytest.mark.parametrize("kd", ["p64", "p32", "res"])
def test_what_the_copy_leaves_alone(monkeypatch, kd):
    """The destination's pose trace, decisions, status flags, chain counters and Joseph setting;
    everything of the source."""
    import torch
    N = 31
    src = _handle(monkeypatch, "p64", N)
    odom = _populate(src, N)
    src.trace_enable(4)
    dst, twin, simple = (_handle(monkeypatch, kd, N, var=DST_VAR) for _ in range(3))
    cnt, ids, act, rel, od = _messages(N, 1)
    dst.trace_enable(8)
    assert dst.set_joseph(True) == twin.set_joseph(True) == pyekf.EKF_OK
    c = int(cnt[0, 0])
    assert dst.set_odom(od[0, 0]) == 0
    rc, j, nw = dst.sensor(rel[0, 0, :c])  # (decisions and a trace record)
    assert rc == 0
    # a status flag: a device-input message whose id is outside the map
    bad = [torch.from_numpy(np.ascontiguousarray(a)).cuda()
           for a in (cnt[1:2], np.full_like(ids[1:2], N), act[1:2], rel[1:2], od[1:2])]
    dst.replay_on_device(bad[0], bad[3], bad[4], ids=bad[1], actions=bad[2])
    dst.sync()
    keep = (dst.trace_count(), dst.trace()[0].copy(), dst.trace()[1].copy(), dst.decisions(c),
            dst.chain_path_counts())
    s_before = (_snap(src), src.trace_count())
    dst.copy_state_from(src, 0, 0)
    assert dst.trace_count() == keep[0] >= 1
    np.testing.assert_array_equal(dst.trace()[0], keep[1])
    np.testing.assert_array_equal(dst.trace()[1], keep[2])
    np.testing.assert_array_equal(dst.decisions(c), keep[3])
    assert dst.chain_path_counts() == keep[4]
    assert dst.status() == pyekf.EKF_FLAG_RANGE
    _same(_snap(src), s_before[0], "the source:")
    assert src.trace_count() == s_before[1] and src.status() == 0
    # the Joseph setting: the next messages run in that form
    _host_route(twin, 0, src, 0, odom[0])
    _host_route(simple, 0, src, 0, odom[0])
    for e in (dst, twin, simple):
        _continue(e, N, [0])
    _same(_snap(dst), _snap(twin), "Joseph form:")
    # (the two forms differ by the rounding of V·Kᵀ, V = ΣHᵀ − K·S ≈ 0 at fp64's level: an fp32 Σ
    # does not hold the difference, so only the fp64 kinds can tell the forms apart)
    if kd != "p32":
        assert not np.array_equal(dst.state()[1], simple.state()[1])
    _close(src, dst, twin, simple)


@pytest.mark.parametrize("ks,ns,nd", [("res", 31, 63), ("p32", 63, 63), ("p64", 30, 31)])
def test_lds_left_by_another_kernel(monkeypatch, ks, ns, nd):
    """An fp64 pipeline destination transposes through LDS: poisoned first, same bits."""
    src = _handle(monkeypatch, ks, ns)
    odom = _populate(src, ns)
    dst, twin = (_handle(monkeypatch, "p64", nd, var=DST_VAR) for _ in range(2))
    src.sync()
    pyekf.poison_lds()
    dst.copy_state_from(src, 0, 0)
    _host_route(twin, 0, src, 0, odom[0])
    _same(_snap(dst), _snap(twin))
    _close(src, dst, twin)


def test_errors_change_nothing(monkeypatch):
    L, E = pyekf.lib(), pyekf.EKF_E_ARG
    big = _handle(monkeypatch, "p64", 31, F=3)
    small = _handle(monkeypatch, "p32", 30, F=3, var=DST_VAR)
    two = _handle(monkeypatch, "res", 31, F=2, var=DST_VAR)
    for h, N in ((big, 31), (small, 30), (two, 31)):
        _populate(h, N, slice(0, 3))
    before = [_snap(h) for h in (big, small, two)]
    assert L.ekf_copy_state(small.h, 0, big.h, 0) == E      # N_dst < N_src
    assert L.ekf_copy_state(small.h, -1, big.h, -1) == E
    assert L.ekf_copy_state(two.h, -1, big.h, -1) == E      # unequal F in the swarm form
    assert L.ekf_copy_state(big.h, -1, two.h, -1) == E
    assert L.ekf_copy_state(big.h, 1, small.h, -1) == E     # one destination, every source
    assert L.ekf_copy_state(big.h, 3, small.h, 0) == E      # indices out of range
    assert L.ekf_copy_state(big.h, 0, small.h, 3) == E
    assert L.ekf_copy_state(two.h, 2, big.h, 0) == E
    assert L.ekf_copy_state(two.h, 0, big.h, 7) == E
    assert L.ekf_copy_state(None, 0, big.h, 0) == E
    assert L.ekf_copy_state(big.h, 0, None, 0) == E
    for h, b in zip((big, small, two), before):
        _same(_snap(h), b)
    assert L.ekf_copy_state(big.h, 0, small.h, 0) == pyekf.EKF_OK   # (and the handles still work)
    assert L.ekf_copy_state(two.h, -1, big.h, 1) == pyekf.EKF_OK
    _close(big, small, two)
