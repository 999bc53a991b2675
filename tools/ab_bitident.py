"""Dev tool: is a rebuilt library bit-identical to a reference build on the GPU?

  python tools/ab_bitident.py <libA.so> <libB.so>   (names inside ekf-slam_amd/, EKF_LIB)

Each library runs the same replays in its own child process (the headline fp32 N = 1024 device
replay from an fp64 survey, fp64 N = 1024, messages of two chunks, the Joseph form, the rebuild
without staged operands, wave 0's lean program (EKF_CHAIN_FAST=1), the Joseph form in
fp32 and under unknown association, four filters with
event hand-offs, unknown association and its routes: one marker per launch, one workgroup, three
on each transport, a map that fills, messages of two chunks; the resident kernel: full maps in each
register layout, known ids and association, a map that fills, the Joseph form, a ragged 48-filter
handle, a replay across staging blocks and flushes, the per-call surface); the final states are
compared bit for bit. A pure
performance change of the kernels (same formulas, same summation order) must print "identical"."""
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "gpurun_out")


def child(tag):
    sys.path.insert(0, os.path.join(ROOT, "ekf-slam_amd"))
    import pyekf
    from pyekf import synth
    res = {}
    # EKF_CHAIN_FAST set by the caller: every leg's setting unless the leg sets its own (unset: each
    # library's default, which differs between builds from before and after the lean program
    # became the default)
    fast = os.environ.get("EKF_CHAIN_FAST")

    def env(**kv):
        for k in ("EKF_SERIAL", "EKF_DEVSYNC", "EKF_STAGE", "EKF_CU_SPLIT", "EKF_RESIDENT",
                  "EKF_AM_XCD", "EKF_ASSOC_MSG", "EKF_CHAIN_FAST"):
            os.environ.pop(k, None)
        if fast is not None:
            os.environ["EKF_CHAIN_FAST"] = fast
        os.environ.update(kv)

    def keep(name, e, F=1):
        for f in range(F):
            x, S, c = e.state(f)
            res[f"{name}_x{f}"], res[f"{name}_S{f}"] = x, S
            res[f"{name}_st{f}"] = np.array([e.status(f), c])

    def stack(scs, T, assoc):
        """Filter f = scenario f, ragged: replay()'s counts, rel, odom, ids (None: unknown),
        actions."""
        F, M = len(scs), max(s.ids.shape[1] for s in scs)
        counts, ids = np.zeros((T, F), np.int32), np.full((T, F, M), -1, np.int32)
        act, rel, odom = np.zeros((T, F, M), np.int32), np.zeros((T, F, M, 2)), np.zeros((T, F, 3))
        for f, s in enumerate(scs):
            m = s.ids.shape[1]
            counts[:, f], ids[:, f, :m] = s.count, s.ids
            act[:, f, :m], rel[:, f, :m] = s.actions, s.rel
            odom[:, f] = pyekf.odometry(s)
        return counts, rel, odom, None if assoc else ids, act

    # headline: fp64 survey, then fp32 N = 1024 through the device planner, and fp64 host-planned
    env()
    N, warm, T = 1024, 40, 24
    sc = synth.synthetic(N, warm + T)
    odom = pyekf.odometry(sc)
    e64 = pyekf.EKF(n_landmarks=N)
    e64.replay(sc.count[:warm, None], sc.rel[:warm, None], odom[:warm, None],
               ids=sc.ids[:warm, None], actions=sc.actions[:warm, None])
    x0, S0, c0 = e64.state()
    tmo = e64.map_odom()
    keep("survey64", e64)
    sl = slice(warm, warm + T)
    e64.replay(sc.count[sl, None], sc.rel[sl, None], odom[sl, None], ids=sc.ids[sl, None],
               actions=sc.actions[sl, None])
    keep("n1024_f64", e64)
    e64.close()
    import torch
    g = [torch.from_numpy(np.ascontiguousarray(a[sl, None])).cuda() for a in
         (sc.count, sc.ids, sc.actions, sc.rel, odom)]
    e = pyekf.EKF(n_landmarks=N, dtype=pyekf.EKF_F32)
    e.set_state(x0, S0, tmo=tmo, counter=c0)
    e.replay_device(g[0], g[3], g[4], g[1], g[2])
    keep("n1024_f32_dev", e)
    e.close()
    # messages of two chunks, fp64, device epochs and events
    sc = synth.synthetic(96, 14, max_markers=24)
    odom = pyekf.odometry(sc)
    for name, kv in (("multi_dev", {}), ("multi_evt", {"EKF_DEVSYNC": "0"})):
        env(**kv)
        e = pyekf.EKF(n_landmarks=96)
        e.replay(sc.count[:, None], sc.rel[:, None], odom[:, None], ids=sc.ids[:, None],
                 actions=sc.actions[:, None])
        keep(name, e)
        e.close()
    # Joseph
    env()
    e = pyekf.EKF(n_landmarks=96)
    e.set_joseph(True)
    e.replay(sc.count[:, None], sc.rel[:, None], odom[:, None], ids=sc.ids[:, None],
             actions=sc.actions[:, None])
    keep("joseph", e)
    e.close()
    # k_chain branches the legs above leave out, on the same messages. The rebuild from operands
    # the chain gathers itself (EKF_STAGE=0: no staged image, store_raw_image) ...
    for name, dt in (("nostage64", pyekf.EKF_F64), ("nostage32", pyekf.EKF_F32)):
        env(EKF_STAGE="0")
        e = pyekf.EKF(n_landmarks=96, dtype=dt)
        e.replay(sc.count[:, None], sc.rel[:, None], odom[:, None], ids=sc.ids[:, None],
                 actions=sc.actions[:, None])
        keep(name, e)
        e.close()
    # ... common-case corrections in wave 0's lean program, the generic one resumed in mid-chunk
    # at each first sighting (EKF_CHAIN_FAST=1; a library from before the two programs ignores
    # the switch) ...
    for name, dt, jo in (("lean64", pyekf.EKF_F64, False), ("lean32", pyekf.EKF_F32, False),
                         ("lean_joseph32", pyekf.EKF_F32, True)):
        env(EKF_CHAIN_FAST="1")
        e = pyekf.EKF(n_landmarks=96, dtype=dt)
        e.set_joseph(jo)
        e.replay(sc.count[:, None], sc.rel[:, None], odom[:, None], ids=sc.ids[:, None],
                 actions=sc.actions[:, None])
        keep(name, e)
        e.close()
    # ... the Joseph form in fp32 (its pend patch carries the V·Kᵀ term) ...
    env()
    e = pyekf.EKF(n_landmarks=96, dtype=pyekf.EKF_F32)
    e.set_joseph(True)
    e.replay(sc.count[:, None], sc.rel[:, None], odom[:, None], ids=sc.ids[:, None],
             actions=sc.actions[:, None])
    keep("joseph32", e)
    e.close()
    # ... and unknown association with the Joseph form on (kNoInit chunks of the Joseph chain)
    for name, dt in (("assoc_joseph64", pyekf.EKF_F64), ("assoc_joseph32", pyekf.EKF_F32)):
        e = pyekf.EKF(n_landmarks=96, dtype=dt)
        e.set_joseph(True)
        e.replay(sc.count[:, None], sc.rel[:, None], odom[:, None], ids=None,
                 actions=sc.actions[:, None], assoc=True)
        keep(name, e)
        e.close()
    # four filters, N = 256, events; and one stream
    sc = synth.synthetic(256, 20)
    odom = pyekf.odometry(sc)
    rep = lambda a: np.ascontiguousarray(np.repeat(a[:, None], 4, 1))  # noqa: E731
    for name, kv in (("f4_evt", {"EKF_DEVSYNC": "0"}), ("f4_ser", {"EKF_SERIAL": "1"})):
        env(**kv)
        e = pyekf.EKF(n_landmarks=256, n_filters=4)
        e.replay(rep(sc.count), rep(sc.rel), rep(odom), ids=rep(sc.ids), actions=rep(sc.actions))
        keep(name, e, 4)
        e.close()
    # unknown association (sensor_cb), fp64 and fp32
    env()
    sc = synth.synthetic(96, 20, shuffle=True)
    odom = pyekf.odometry(sc)
    for name, dt in (("assoc64", pyekf.EKF_F64), ("assoc32", pyekf.EKF_F32)):
        e = pyekf.EKF(n_landmarks=96, dtype=dt)
        e.replay(sc.count[:, None], sc.rel[:, None], odom[:, None], ids=None,
                 actions=sc.actions[:, None], assoc=True)
        keep(name, e)
        e.close()
    # k_assoc_msg's and k_assoc's branches the legs above leave out, fp64 and fp32 each
    def assoc_leg(name, N, sc, **kv):
        env(**kv)
        odom = pyekf.odometry(sc)
        for sfx, dt in (("64", pyekf.EKF_F64), ("32", pyekf.EKF_F32)):
            e = pyekf.EKF(n_landmarks=N, dtype=dt)
            e.replay(sc.count[:, None], sc.rel[:, None], odom[:, None], ids=None,
                     actions=sc.actions[:, None], assoc=True)
            keep(name + sfx, e)
            e.close()

    # ... the one-marker route (k_assoc) on the messages above ...
    assoc_leg("assoc_marker", 96, sc, EKF_ASSOC_MSG="0")
    # ... one workgroup on the pipeline (G == 1: v_readlane instead of the tables) ...
    sc20 = synth.make_scenario(20, synth.random_landmarks(12, seed=7), 10, max_markers=16, seed=14,
                               shuffle=True)
    assoc_leg("assoc_1wg", 20, sc20, EKF_RESIDENT="0", EKF_AM_XCD="0")
    # ... three workgroups on each transport ...
    sc130 = synth.make_scenario(130, synth.random_landmarks(100, seed=11), 10, max_markers=16,
                                seed=18, shuffle=True)
    assoc_leg("assoc_3wg_xcd", 130, sc130, EKF_AM_XCD="1")
    assoc_leg("assoc_3wg_agent", 130, sc130, EKF_AM_XCD="0")
    # ... a map that fills during the run (the drives sight 8 / 130 landmarks, the filters hold
    # 3 / 70: later markers are skipped with EKF_FLAG_RANGE), one and two workgroups ...
    assoc_leg("assoc_fill_1wg", 3, synth.make_scenario(8, synth.random_landmarks(8, seed=9), 12,
                                                       max_markers=8, seed=10, shuffle=True),
              EKF_RESIDENT="0")
    assoc_leg("assoc_fill_2wg", 70, synth.populated(130, 6, shuffle=True), EKF_RESIDENT="0")
    # ... and messages of two chunks (24 markers) under association
    assoc_leg("assoc_multi", 96, synth.synthetic(96, 14, max_markers=24, shuffle=True))
    # k_resident (fp64, n ≤ 128): every instantiation and branch. Full maps at N = 50 (26 row
    # slots), 51 and 62 (32), known ids and association; N = 30 (16 row slots, one column slot)
    # under association, where the map fills (EKF_FLAG_RANGE); the Joseph form at N = 30, 50, 62
    def resident_leg(name, N, assoc, joseph=False):
        env(EKF_RESIDENT="1")
        sc = synth.populated(N, 6, shuffle=assoc)
        odom = pyekf.odometry(sc)
        e = pyekf.EKF(n_landmarks=N)
        assert e.path == pyekf.EKF_PATH_RESIDENT
        if joseph:
            e.set_joseph(True)
        e.replay(sc.count[:, None], sc.rel[:, None], odom[:, None],
                 ids=None if assoc else sc.ids[:, None], actions=sc.actions[:, None], assoc=assoc)
        keep(name, e)
        e.close()

    for N in (50, 51, 62):
        resident_leg(f"res_full{N}_known", N, False)
        resident_leg(f"res_full{N}_assoc", N, True)
    resident_leg("res_fill30_assoc", 30, True)
    for N in (30, 50, 62):  # the Joseph instantiation of each layout: 16/1, 26/2, 32/2
        resident_leg(f"res_joseph{N}_known", N, False, joseph=True)
        resident_leg(f"res_joseph{N}_assoc", N, True, joseph=True)
    # ... 48 filters with different maps and ragged messages in one handle, one upload ...
    F, T, N = 48, 24, 40
    for assoc in (False, True):
        scs = [synth.make_scenario(N, synth.random_landmarks(10 + f % 20, seed=300 + f), T,
                                   max_markers=4 + f % 9, seed=400 + f, shuffle=assoc)
               for f in range(F)]
        e = pyekf.EKF(n_landmarks=N, n_filters=F)
        e.replay(*stack(scs, T, assoc), assoc=assoc)
        keep("res_ragged_" + ("assoc" if assoc else "known"), e, F)
        e.close()
    # ... a replay of 40 messages × 256 filters: several 16-entry staging blocks per launch, and
    # the plan is flushed every 8192 descriptors (Σ leaves the registers and comes back) ...
    F, T, N = 256, 40, 24
    base = [synth.synthetic(N, T, seed=500 + k, max_markers=8) for k in range(4)]
    e = pyekf.EKF(n_landmarks=N, n_filters=F)
    e.replay(*stack([base[f % 4] for f in range(F)], T, False))
    keep("res_spans_uploads", e, F)
    e.close()
    # ... and the per-call surface, one launch each: predict / correct / posterior on the known-id
    # golden drive, predict / associate_correct / posterior on the association one
    for gname in ("basic_world_known", "basic_world_assoc"):
        g = np.load(os.path.join(ROOT, "tests", "golden", gname + ".npz"))
        sc = synth.Scenario(int(g["n_landmarks"]), g["landmarks"], g["wheel"], g["ids"],
                            g["actions"], g["rel"], g["count"], g["truth"], float(g["track"]),
                            float(g["radius"]))
        odom = pyekf.odometry(sc)
        e = pyekf.EKF(n_landmarks=sc.n_landmarks)
        dec = []
        for t in range(sc.n_messages):
            e.set_odom(odom[t])
            e.predict()
            for i in range(int(sc.count[t])):
                if bool(g["assoc"]):
                    dec.append(e.associate_correct(*sc.rel[t, i]))
                elif sc.actions[t, i] == 0:
                    e.correct(int(sc.ids[t, i]), *sc.rel[t, i])
            e.posterior()
        keep("res_percall_" + gname, e)
        res["res_percall_dec_" + gname] = np.array(dec, dtype=np.int64)
        res["res_percall_tmo_" + gname] = np.asarray(e.map_odom())
        e.close()
    env()
    # digests only (a whole fp64 Σ at N = 1024 is 34 MB): bit-identical ⇔ equal digests
    import hashlib
    import json
    dig = {k: [hashlib.sha256(np.ascontiguousarray(v).tobytes()).hexdigest(),
               float(np.nansum(np.abs(v.astype(float))))] for k, v in res.items()}
    os.makedirs(OUT, exist_ok=True)
    with open(os.path.join(OUT, f"ab_{tag}.json"), "w") as fh:
        json.dump(dig, fh)


def main():
    if len(sys.argv) == 3 and sys.argv[1] == "--child":
        return child(sys.argv[2])
    a, b = sys.argv[1], sys.argv[2]
    for lib in (a, b):
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", lib],
                           env=dict(os.environ, EKF_LIB=lib), timeout=600)
        if r.returncode:
            print(f"child {lib} failed: rc {r.returncode}")
            return r.returncode
    import json
    A = json.load(open(os.path.join(OUT, f"ab_{a}.json")))
    B = json.load(open(os.path.join(OUT, f"ab_{b}.json")))
    bad = [f"{k}: sum|v| {A[k][1]:.17g} vs {B[k][1]:.17g}" for k in A if A[k][0] != B.get(k, [""])[0]]
    print("identical" if not bad else "DIFFER:\n  " + "\n  ".join(bad))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
