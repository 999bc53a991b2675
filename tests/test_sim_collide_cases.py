"""The collision cases of tests/sim_collide_cases.py, pinned on pyekf.synth's output alone (no GPU):
each case reaches the path it is named for, is decidable (no executed test d < R within GAP = 1e-6 of
a different answer; the markers under sim_cases.guard), the analytic head-on result holds, a scalar
tick-by-tick walk written here from the rule's text (nusim.cpp:232-254) gives synth._simulate's
poses and counts, and synth._simulate without the new arguments is bit-equal to the loop it was
before them, restated here (on the inputs of tests/sim_cases.py, whose Swarms are built without
them).
"""
import math

import numpy as np
import pytest

import sim_cases as sc
import sim_collide_cases as cc
from pyekf import synth

R = cc.R


def simulate_before(drive, seeds, start_pose, slip):
    """synth._simulate as it stood before the collision arguments, restated here so that the pin
    below does not go through the code it pins: the commanded increments, the slip draws, one
    _fkin_step per tick from the accumulated wheel angles. → (wheel, truth, path)."""
    F, nt, tpm = seeds.shape[0], drive.v.shape[0], drive.ticks_per_msg
    T, dt = nt // tpm, 1.0 / drive.tick_hz
    wr = (drive.v + drive.w * synth.TRACK_WIDTH / 2.0) / synth.WHEEL_RADIUS * dt
    wl = (drive.v - drive.w * synth.TRACK_WIDTH / 2.0) / synth.WHEEL_RADIUS * dt
    cmd = np.stack([wl, wr], 1)
    wheel = np.cumsum(cmd, 0).reshape(T, tpm, 2)
    k = np.arange(nt, dtype=np.uint64)
    u = synth.rng_uniform(seeds[:, None, None], synth._S_SLIP,
                          (k[None, :, None] * np.uint64(2) + np.arange(2, dtype=np.uint64)))
    slipped = cmd[None] * (1.0 + slip * (2.0 * u - 1.0))
    config = tuple(np.full(F, float(v)) for v in start_pose)
    phi_l, phi_r = np.zeros(F), np.zeros(F)
    path, truth = np.zeros((F, nt, 2)), np.zeros((F, T, 3))
    for i in range(nt):
        nl, nr = phi_l + slipped[:, i, 0], phi_r + slipped[:, i, 1]
        config = synth._fkin_step(config, nl - phi_l, nr - phi_r)
        phi_l, phi_r = nl, nr
        path[:, i, 0], path[:, i, 1] = config[1], config[2]
        if (i + 1) % tpm == 0:
            truth[:, (i + 1) // tpm - 1] = np.stack(config, 1)
    return wheel, truth, path


def walk(case, f):
    """The rule, scalar and tick by tick, for filter f: FKin by synth._fkin_step, then the
    landmarks in id order with math.sqrt / atan2 / cos / sin. → (truth [T, 3], per tick: the ids the
    pose was inside before the push, the id that acted or −1, the pose after the tick)."""
    sw = case.sw
    T, tpm = sw.count.shape[0], sw.wheel.shape[1]
    lm = sw.landmarks[f]
    k = np.arange(T * tpm, dtype=np.uint64)
    u = synth.rng_uniform(sw.seeds[f], synth._S_SLIP,
                          k[:, None] * np.uint64(2) + np.arange(2, dtype=np.uint64))
    inc = sw.cmd * (1.0 + case.sim_kw["slip"] * (2.0 * u - 1.0))
    cfg = tuple(np.array([float(v)]) for v in sw.start_pose)
    phi = [np.zeros(1), np.zeros(1)]
    truth, ticks = np.zeros((T, 3)), []
    for i in range(T * tpm):
        nl, nr = phi[0] + inc[i, 0], phi[1] + inc[i, 1]
        cfg = synth._fkin_step(cfg, nl - phi[0], nr - phi[1])
        phi = [nl, nr]
        th, x, y = (float(v[0]) for v in cfg)
        inside, acted = [], -1
        for l in range(lm.shape[0]):
            lx, ly = float(lm[l, 0]), float(lm[l, 1])
            if math.sqrt((x - lx) * (x - lx) + (y - ly) * (y - ly)) < R:
                inside.append(l)
        if inside:
            acted = inside[0]
            lx, ly = float(lm[acted, 0]), float(lm[acted, 1])
            d = math.sqrt((x - lx) * (x - lx) + (y - ly) * (y - ly))
            a = math.atan2(ly - y, lx - x)
            x, y = x - (R - d) * math.cos(a), y - (R - d) * math.sin(a)
            cfg = (cfg[0], np.array([x]), np.array([y]))
        ticks.append((inside, acted, (th, x, y)))
        if (i + 1) % tpm == 0:
            truth[(i + 1) // tpm - 1] = (th, x, y)
    return truth, ticks


@pytest.mark.parametrize("name", cc.NAMES)
def test_case_is_decidable_and_restated(name):
    c = cc.get(name)
    sw = c.sw
    edge = cc.guard(c)
    print(f"{name}: smallest |d - R| {edge:.3g}, hits per message {sw.hits.sum(1).tolist()}")
    T, F = sw.count.shape
    tpm = sw.wheel.shape[1]
    assert T <= 8 and F <= 2 and c.parallel
    assert sw.hits.shape == (T, F) and sw.hits.dtype == np.int32
    assert c.collision_radius + c.obstacle_radius == R
    # the runs tile the drive; the Sim keywords reproduce the Swarm
    assert c.bounds[0][0] == 0 and c.bounds[-1][1] == T
    assert all(a[1] == b[0] for a, b in zip(c.bounds, c.bounds[1:]))
    assert (sw.seeds == np.uint64(c.sim_kw["seed"]) + np.arange(F, dtype=np.uint64)).all()
    assert tpm == c.sim_kw["ticks_per_msg"] and sw.cmd.shape[0] == T * tpm
    assert c.stride == c.sim_kw["marker_stride"] and c.n_map <= c.n_slots
    assert tuple(sw.start_pose) == (c.sim_kw["start_theta"], c.sim_kw["start_x"],
                                    c.sim_kw["start_y"])
    # the scalar walk against the vectorised restatement: libm against numpy, a few ulp a tick
    truth, path, hits, edge2 = cc.simulate(c)
    assert edge2 == sw.hit_edge
    np.testing.assert_array_equal(hits.T, sw.hits)
    np.testing.assert_array_equal(truth.transpose(1, 0, 2), sw.truth)
    for f in range(F):
        wt, ticks = walk(c, f)
        assert np.abs(wt - sw.truth[:, f]).max() < 1e-12
        per_msg = np.array([a >= 0 for _, a, _ in ticks]).reshape(T, tpm).sum(1)
        np.testing.assert_array_equal(per_msg, sw.hits[:, f])
        np.testing.assert_allclose(np.array([p[1:] for _, _, p in ticks]), path[f], atol=1e-12)
    if name != "clear":
        assert sw.hits.sum() > 0


def _ticks(name, f=0):
    c = cc.get(name)
    return c, walk(c, f)[1]


def test_head_on_is_held_at_the_cylinder_while_odometry_goes_on():
    c = cc.get("head-on")
    sw = c.sw
    cx = float(sw.landmarks[0, 0, 0])
    th, x, y = sw.truth[-1, 0]
    assert abs(x - (cx - R)) < 1e-12 and y == 0.0 and th == 0.0
    from pyekf import odometry
    odo = odometry(sw.scenario(0))
    assert abs(odo[-1][1] - 8 * 40 * cc.STEP) < 1e-9          # 0.8 m commanded
    assert odo[-1][1] - x > 0.4
    # every tick from the first contact on collides
    first = int(np.argmax(sw.hits[:, 0] > 0))
    assert 0 < sw.hits[first, 0] <= 40 and (sw.hits[first + 1:, 0] == 40).all()


def test_glance_slides_round_and_leaves():
    c, ticks = _ticks("glance")
    acted = np.array([a for _, a, _ in ticks])
    hit = np.flatnonzero(acted >= 0)
    assert len(hit) >= 10 and (np.diff(hit) == 1).all()        # consecutive ticks
    assert hit[-1] < len(ticks) - 40                           # and a free message after it
    assert c.sw.hits[-1, 0] == 0
    # it left below the cylinder: the y of a pose at distance R under the centre, x past it
    th, x, y = c.sw.truth[-1, 0]
    assert th == 0.0 and x > 0.5 and abs(y - (0.1 - R)) < 1e-3


@pytest.mark.parametrize("name,tick", [("first-tick", 80), ("last-tick", 79)])
def test_first_contact_falls_on_the_named_tick(name, tick):
    c, ticks = _ticks(name)
    acted = [a for _, a, _ in ticks]
    assert acted.index(0) == tick and all(a == 0 for a in acted[tick:])
    assert c.sw.wheel.shape[1] == 40
    t, j = divmod(tick, 40)
    assert j == (0 if name == "first-tick" else 39)
    assert c.sw.hits[:, 0].tolist() == [0] * t + [40 - j] + [40] * (c.sw.count.shape[0] - t - 1)


def test_contact_carries_over_a_message_and_a_run_boundary():
    c = cc.get("over-message")
    h = c.sw.hits[:, 0]
    t = int(np.argmax(h > 0))
    assert 0 < h[t] < 40 and h[t + 1] > 0 and h[-1] == 0     # begins inside a message, goes on, ends
    _, ticks = _ticks("over-message")
    acted = [a for _, a, _ in ticks]
    assert acted[40 * (t + 1) - 1] == 0 and acted[40 * (t + 1)] == 0        # across the boundary
    c = cc.get("run-split")
    assert len(c.bounds) == 2
    cut = c.bounds[0][1]
    assert c.sw.hits[cut - 1, 0] == 40 and c.sw.hits[cut, 0] == 40          # in contact at the cut


def test_ticks_cases():
    c = cc.get("ticks-1")
    assert c.sw.wheel.shape[1] == 1 and c.sw.hits[:, 0].tolist() == [0, 0, 1, 1, 1, 1, 1, 1]
    c = cc.get("ticks-64")
    assert c.sw.wheel.shape[1] == 64
    h = c.sw.hits[:, 0]
    assert (h > 0).sum() >= 2 and h[-1] == 0 and h.max() < 64


@pytest.mark.parametrize("name,low,high", [("map-65", 3, 64), ("map-1024", 700, 1023)])
def test_map_cases_lowest_id_wins(name, low, high):
    c, ticks = _ticks(name)
    assert c.n_map == int(name.split("-")[1])
    assert low % 64 != high % 64 and low // 64 != high // 64 and low < high
    alone = [a for ins, a, _ in ticks if ins == [high]]
    both = [a for ins, a, _ in ticks if ins == [low, high]]
    assert alone and set(alone) == {high}                       # the higher id is hit first, alone
    assert both and set(both) == {low}                          # inside both: the lower acts
    first_high = next(i for i, (ins, _, _) in enumerate(ticks) if ins)
    assert ticks[first_high][0] == [high]
    assert all(set(ins) <= {low, high} for ins, _, _ in ticks)  # no other landmark is ever hit
    assert cc.get("map-1").n_map == 1


def test_start_inside_and_chain_break_the_lists_bound():
    """Both push the pose further from the message's start than ρ, the reach the candidate list of
    that message was built for: the kernel must rebuild it (its header comment)."""
    c, ticks = _ticks("start-inside")
    assert ticks[0][1] == 0                                     # tick 0 is inside
    th, x, y = ticks[0][2]
    assert math.hypot(x, y) > 0.09 and c.sw.hits[0, 0] >= 1

    c, ticks = _ticks("chain")
    tpm = c.sw.wheel.shape[1]
    rho = cc.rho(c)
    assert rho.shape == c.sw.hits.shape and abs(rho[0, 0] - tpm * cc.STEP) < 1e-6
    acted = [a for _, a, _ in ticks[:tpm]]
    assert acted == list(range(8))                              # handed from one to the next
    start = np.array(c.sw.start_pose[1:])
    disp = [math.hypot(p[1] - start[0], p[2] - start[1]) for _, _, p in ticks[:tpm]]
    assert disp[0] > rho[0, 0] and disp[-1] > 0.3 > 10 * rho[0, 0]
    # the last links lie beyond the first list's reach ρ + R about the start
    far = np.hypot(*(c.sw.landmarks[0, :8] - start).T) > rho[0, 0] + R
    assert far[6:].all() and not far[:4].any()
    assert c.sw.hits[:, 0].tolist() == [8, 0, 0, 0, 0, 0]


def test_one_of_two_and_clear():
    c = cc.get("one-of-two")
    assert c.sw.n_filters == 2
    assert c.sw.hits[:, 0].sum() > 0 and c.sw.hits[:, 1].sum() == 0
    c = cc.get("clear")
    assert c.sw.hits.sum() == 0 and c.sw.hit_edge > 0.1
    base = sc.get("size-64").sw
    # nothing hit: the poses and markers of the run without collisions, bit for bit
    for a, b in ((c.sw.truth, base.truth), (c.sw.rel, base.rel), (c.sw.ids, base.ids)):
        assert a.tobytes() == b.tobytes()


def test_simulate_without_the_new_arguments_is_unchanged():
    """The three-value return and the bits of the earlier _simulate (simulate_before above), with
    the collision arguments left out and with them given but a zero collision radius; and the
    sim_cases Swarms, built through the defaults, carry those bits and no collision fields."""
    for name in ("size-64", "ticks-63", "mixed-all", "f0-seed", "no-noise"):
        case = sc.get(name)
        sw = case.sw
        T, tpm = sw.count.shape[0], sw.wheel.shape[1]
        drive = synth.circle_drive(T, 1.0, 0.5, 200.0, tpm)
        want = simulate_before(drive, sw.seeds, sw.start_pose, case.sim_kw["slip"])
        out = synth._simulate(drive, sw.seeds, sw.start_pose, case.sim_kw["slip"])
        off = synth._simulate(drive, sw.seeds, sw.start_pose, case.sim_kw["slip"], sw.landmarks,
                              0.0, 0.038)
        for o in (out, off):
            assert len(o) == 3
            for got, ref in zip(o, want):
                assert got.shape == ref.shape and got.tobytes() == ref.tobytes(), name
        assert sw.wheel.tobytes() == want[0].tobytes()
        assert sw.truth.tobytes() == np.ascontiguousarray(want[1].transpose(1, 0, 2)).tobytes()
        assert sw.hits is None and sw.hit_edge == math.inf
