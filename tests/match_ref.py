"""The matching of ekf_eval_match (ekf-slam_amd/csrc/match_math.hpp, k_eval_match in ekf_eval.hip)
restated in numpy, operation for operation: numpy rounds every product and sum on its own, as the
library does (-ffp-contract=off), so the squared distances have the same bits and the matches and
the record compare exactly. Shared by the host and the GPU tests of the matching."""
import numpy as np

import pyekf


def seen_slots(xy):
    return ~((xy[:, 0] == 0.0) & (xy[:, 1] == 0.0))


def sq_distances(xy, truth_map):
    """d2[j, k] = dx*dx + dy*dy of slot j to truth k (both in the map frame); +inf where it is NaN
    (a NaN truth never wins) ."""
    with np.errstate(invalid="ignore", over="ignore"):
        dx = xy[:, None, 0] - truth_map[None, :, 0]
        dy = xy[:, None, 1] - truth_map[None, :, 1]
        d2 = dx * dx + dy * dy
    return np.where(np.isnan(d2), np.inf, d2)


def match_np(xy, truth_map, max_dist, truth_raw=None):
    """xy [N, 2]: the slots' estimates; truth_map [n_map, 2]: the truth in the map frame;
    truth_raw: the truth as given (n_truth counts its landmarks without a NaN), by default
    truth_map. Returns (match [N] int32, record of MATCH_DTYPE, best d2 [N], second-best d2 [N])."""
    xy = np.asarray(xy, np.float64)
    truth_map = np.asarray(truth_map, np.float64)
    raw = truth_map if truth_raw is None else np.asarray(truth_raw, np.float64)
    N = len(xy)
    seen = seen_slots(xy)
    d2 = sq_distances(xy, truth_map)
    k = d2.argmin(1)                      # the first minimum: a strict < scan in ascending k
    best = d2[np.arange(N), k]
    gate2 = np.float64(max_dist) * np.float64(max_dist)
    matched = seen & (best < np.inf) & (best <= gate2)
    match = np.where(matched, k, -1).astype(np.int32)
    second = np.sort(d2, 1)[:, 1] if d2.shape[1] > 1 else np.full(N, np.inf)
    rec = np.zeros((), pyekf.MATCH_DTYPE)
    rec["n_truth"] = int((~np.isnan(raw).any(1)).sum())
    rec["n_matched"] = int(matched.sum())
    owners = {}
    for j in np.flatnonzero(matched):     # ascending: the first slot of a landmark is its lowest
        owners.setdefault(int(match[j]), int(j))
    rec["n_primary"] = len(owners)
    rec["n_dup"] = rec["n_matched"] - rec["n_primary"]
    rec["n_spurious"] = int(seen.sum()) - rec["n_matched"]
    rec["n_missed"] = rec["n_truth"] - rec["n_primary"]
    rec["max_match_dist"] = np.sqrt(best[matched].max()) if matched.any() else 0.0
    return match, rec, best, second


def wrap(a):
    """geom.hpp's normalize_angle: into (-pi, pi], -pi -> pi."""
    d = np.fmod(np.float64(a) + np.pi, 2.0 * np.pi)
    return d + np.pi if d <= 0.0 else d - np.pi


def to_map_frame(points, frame):
    """eval_math.hpp's truth_point_in_map restated (geom.hpp's inverse and compose, as
    pyekf.synth restates them): the device's sin and cos are within an ulp of numpy's."""
    if frame is None:
        return np.array(points, np.float64)
    from pyekf import synth
    inv = synth._inverse(np.asarray(frame, np.float64))
    out = np.empty_like(np.asarray(points, np.float64))
    for i, p in enumerate(points):
        if np.isnan(p).any():
            out[i] = np.nan
        else:
            out[i] = synth._compose(inv, np.array([0.0, p[0], p[1]]))[1:]
    return out
