"""numpy restatement of the search stage of ORBmatcher::Fuse(pKF, vpMapPoints, th, bRight = false) (reference
src/ORBmatcher.cc:1244-1408), held bit for bit against the reference's compiled definitions by tests/test_orb_fuse.py
(tests/golden/orb_fuse_reference.npz, scripts/make_orb_fuse_golden.py) before any test relies on it at other sizes.

Per pair: Tcw * p3Dw as Sophus' quaternion action (tests/track_motion_restatement.se3_act), p3Dc(2) < 0.0f, invz = 1 / z in f32,
Pinhole::project = fx * x / z + cx, KeyFrame::IsInImage (>= min && < max), the band 0.8f * min .. 1.2f * max on PO.norm() =
sqrt(c0 + (c1 + c2)), PO.dot(Pn) < 0.5 * dist3D compared in f64, PredictScale through the C library's logf
(tests/track_local_restatement.predict_scale), KeyFrame::GetFeaturesInArea (src/KeyFrame.cc:1179-1229), the level band and the
chi-square gates of :1365-1392 (f32 product, f64 comparison; stereo when mvuRight >= 0), the first minimum in enumeration order.
Every operation is one f32 numpy operation: no contraction.

A key frame is a dict(x, y, octave, u_right, desc, min_x, min_y, grid_w_inv, grid_h_inv, scale_factors, inv_level_sigma2,
log_scale_factor, K4, mbf, bounds4, q_cw, tcw, Ow); points a dict(pos, normal, min_dist, max_dist, desc)."""
import math

import numpy as np

from tests.track_local_restatement import predict_scale, rule
from tests.track_motion_restatement import se3_act

f32 = np.float32
REACHED = ("skipped", "behind", "outside", "too_near", "too_far", "view_angle", "empty_window", "no_candidate", "above_th_low", "candidate")
SKIPPED, BEHIND, OUTSIDE, TOO_NEAR, TOO_FAR, VIEW_ANGLE, EMPTY_WINDOW, NO_CANDIDATE, ABOVE_TH_LOW, CANDIDATE = range(10)
GRID_COLS, GRID_ROWS, TH_LOW = 64, 48, 50
SUB_FACTS = ("dropped_below_level", "dropped_above_level", "dropped_mono_gate", "dropped_stereo_gate", "u_right_zero_stereo_branch",
             "clipped_left", "clipped_right", "clipped_top", "clipped_bottom", "tie_winner_not_lowest_index", "dist3d_zero")
_POP = np.array([bin(i).count("1") for i in range(256)], np.int32)


def grid_of(kf):
    """Frame::AssignFeaturesToGrid (src/Frame.cc:717-752, PosInGrid :1305-1316), which the key frame copies: per cell the key point
    indices in insertion order, and the enumeration (column ix outer, row iy inner) as cell starts + members."""
    x, y = np.asarray(kf["x"], f32), np.asarray(kf["y"], f32)
    with np.errstate(all="ignore"):
        fx = ((x - f32(kf["min_x"])) * f32(kf["grid_w_inv"])).astype(np.float64)
        fy = ((y - f32(kf["min_y"])) * f32(kf["grid_h_inv"])).astype(np.float64)
    # C round(): half away from zero (numpy rounds half to even); the f64 sum with 0.5 is exact
    px = np.where(fx >= 0, np.floor(fx + 0.5), np.ceil(fx - 0.5)).astype(np.int64)
    py = np.where(fy >= 0, np.floor(fy + 0.5), np.ceil(fy - 0.5)).astype(np.int64)
    ok = (px >= 0) & (px < GRID_COLS) & (py >= 0) & (py < GRID_ROWS)
    cell = np.where(ok, px * GRID_ROWS + py, -1)
    idx = np.flatnonzero(ok)
    order = idx[np.argsort(cell[idx], kind="stable")]
    start = np.zeros(GRID_COLS * GRID_ROWS + 1, np.int64)
    np.add.at(start, cell[idx] + 1, 1)
    return np.cumsum(start), order


def front(kf, points):
    """:1294-1337 over all points -> dict(reached (BEHIND .. VIEW_ANGLE, or EMPTY_WINDOW = every test passed), u, v, ur, dist, ratio)."""
    pos, nrm = np.asarray(points["pos"], f32).reshape(-1, 3), np.asarray(points["normal"], f32).reshape(-1, 3)
    K4, b, Ow = np.asarray(kf["K4"], f32), np.asarray(kf["bounds4"], f32), np.asarray(kf["Ow"], f32)
    with np.errstate(all="ignore"):
        pc = se3_act(kf["q_cw"], kf["tcw"], pos).astype(f32)
        behind = pc[:, 2] < 0
        invz = f32(1.0) / pc[:, 2]
        u, v = K4[0] * pc[:, 0] / pc[:, 2] + K4[2], K4[1] * pc[:, 1] / pc[:, 2] + K4[3]
        inside = (u >= b[0]) & (u < b[1]) & (v >= b[2]) & (v < b[3])
        ur = u - f32(kf["mbf"]) * invz
        PO = pos - Ow[None, :]
        dist = np.sqrt(PO[:, 0] * PO[:, 0] + (PO[:, 1] * PO[:, 1] + PO[:, 2] * PO[:, 2]))
        near = dist < f32(0.8) * np.asarray(points["min_dist"], f32)
        far = dist > f32(1.2) * np.asarray(points["max_dist"], f32)
        dot = PO[:, 0] * nrm[:, 0] + (PO[:, 1] * nrm[:, 1] + PO[:, 2] * nrm[:, 2])
        graze = (dot.astype(np.float64) < 0.5 * dist.astype(np.float64)) | (dist == 0)
        ratio = np.asarray(points["max_dist"], f32) / dist
    reached = np.full(len(pos), EMPTY_WINDOW, np.int32)
    for mask, code in ((graze, VIEW_ANGLE), (far, TOO_FAR), (near, TOO_NEAR), (~inside, OUTSIDE), (behind, BEHIND)):
        reached[mask] = code
    return dict(reached=reached, u=u.astype(f32), v=v.astype(f32), ur=ur.astype(f32), dist=dist.astype(f32), ratio=ratio.astype(f32),
                dist_zero=(dist == 0))


def window(kf, grid, x, y, r, counters=None):
    """KeyFrame::GetFeaturesInArea(x, y, r): the indices in the reference's order."""
    start, order = grid
    x, y, r = f32(x), f32(y), f32(r)
    mx, my, wi, hi = f32(kf["min_x"]), f32(kf["min_y"]), f32(kf["grid_w_inv"]), f32(kf["grid_h_inv"])
    raw = [int(math.floor(f32(f32(f32(x - mx) - r) * wi))), int(math.ceil(f32(f32(f32(x - mx) + r) * wi))),
           int(math.floor(f32(f32(f32(y - my) - r) * hi))), int(math.ceil(f32(f32(f32(y - my) + r) * hi)))]
    c0, c1, r0, r1 = max(0, raw[0]), min(GRID_COLS - 1, raw[1]), max(0, raw[2]), min(GRID_ROWS - 1, raw[3])
    if c0 >= GRID_COLS or c1 < 0 or r0 >= GRID_ROWS or r1 < 0:
        return np.zeros(0, np.int64)
    if counters is not None:
        counters["clipped_left"] += raw[0] < 0
        counters["clipped_right"] += raw[1] > GRID_COLS - 1
        counters["clipped_top"] += raw[2] < 0
        counters["clipped_bottom"] += raw[3] > GRID_ROWS - 1
    parts = [order[start[ix * GRID_ROWS + r0]:start[ix * GRID_ROWS + r1 + 1]] for ix in range(c0, c1 + 1)]
    mem = np.concatenate(parts) if parts else np.zeros(0, np.int64)
    kx, ky = np.asarray(kf["x"], f32)[mem], np.asarray(kf["y"], f32)[mem]
    return mem[(np.abs(kx - x) < r) & (np.abs(ky - y) < r)]


def search_pair(kf, grid, fr, i, level, desc, th, counters=None):
    """:1340-1408 for point i of `fr` = front(...) -> (reached, bestIdx, bestDist, candidates whose distance was taken)."""
    radius = f32(th) * np.asarray(kf["scale_factors"], f32)[level]
    ind = window(kf, grid, fr["u"][i], fr["v"][i], radius, counters)
    if len(ind) == 0:
        return EMPTY_WINDOW, -1, 256, 0
    u, v, ur = fr["u"][i], fr["v"][i], fr["ur"][i]
    oct_ = np.asarray(kf["octave"], np.int64)[ind]
    kr = np.asarray(kf["u_right"], f32)[ind]
    below, above = oct_ < level - 1, oct_ > level
    band = ~(below | above)
    ex, ey, er = u - np.asarray(kf["x"], f32)[ind], v - np.asarray(kf["y"], f32)[ind], ur - kr
    sig = np.asarray(kf["inv_level_sigma2"], f32)[np.clip(oct_, 0, len(kf["inv_level_sigma2"]) - 1)]
    with np.errstate(all="ignore"):
        e2s, e2m = (ex * ex + ey * ey) + er * er, ex * ex + ey * ey
        stereo = kr >= 0
        drop_s = stereo & ((e2s * sig).astype(np.float64) > 7.8)
        drop_m = ~stereo & ((e2m * sig).astype(np.float64) > 5.99)
    ok = band & ~drop_s & ~drop_m
    if counters is not None:
        counters["dropped_below_level"] += int(below.sum())
        counters["dropped_above_level"] += int(above.sum())
        counters["dropped_stereo_gate"] += int((band & drop_s).sum())
        counters["dropped_mono_gate"] += int((band & drop_m).sum())
        counters["u_right_zero_stereo_branch"] += int((band & (kr == 0)).sum())
    cand = ind[ok]
    if len(cand) == 0:
        return NO_CANDIDATE, -1, 256, 0
    d = _POP[np.bitwise_xor(np.asarray(kf["desc"], np.uint8)[cand], np.asarray(desc, np.uint8)[None, :])].sum(1)
    j = int(np.argmin(d))            # the first minimum
    best, best_idx = int(d[j]), int(cand[j])
    if counters is not None and best <= TH_LOW and (d == best).sum() > 1 and best_idx != cand[d == best].min():
        counters["tie_winner_not_lowest_index"] += 1
    return (CANDIDATE if best <= TH_LOW else ABOVE_TH_LOW), best_idx, best, len(cand)


def fuse_search(kfs, points, skip, th, counters=None, double_overload=False):
    """-> dict of [K, M] arrays: best_idx / best_dist (the entries' outputs), reached, raw_best_idx / raw_best_dist (bestIdx, bestDist
    as the loop left them: -1 / 256 without a candidate), n_dist (Hamming distances taken), level (-1 before PredictScale), ambiguous
    (track_level.hpp's mark), u, v (0 before the projection)."""
    K, M = len(kfs), len(np.asarray(points["min_dist"]))
    o = dict(best_idx=np.full((K, M), -1, np.int32), best_dist=np.full((K, M), -1, np.int32), reached=np.zeros((K, M), np.uint8),
             raw_best_idx=np.full((K, M), -1, np.int32), raw_best_dist=np.full((K, M), 256, np.int32), n_dist=np.zeros((K, M), np.int32),
             level=np.full((K, M), -1, np.int32), ambiguous=np.zeros((K, M), np.uint8), u=np.zeros((K, M), f32), v=np.zeros((K, M), f32))
    if counters is not None:
        for k in REACHED + SUB_FACTS + ("ambiguous",):
            counters.setdefault(k, 0)
    desc = np.asarray(points["desc"], np.uint8).reshape(-1, 32)
    for k, kf in enumerate(kfs):
        grid = grid_of(kf)
        fr = front(kf, points)
        lsf, levels = f32(kf["log_scale_factor"]), len(kf["scale_factors"])
        for i in range(M):
            if skip is not None and skip[k][i]:
                reached = SKIPPED
            else:
                reached = int(fr["reached"][i])
                if reached != BEHIND:
                    o["u"][k, i], o["v"][k, i] = fr["u"][i], fr["v"][i]
                if counters is not None and reached == VIEW_ANGLE and fr["dist_zero"][i]:
                    counters["dist3d_zero"] += 1
                if reached == EMPTY_WINDOW:
                    level = predict_scale(fr["ratio"][i], lsf, levels, double_overload)[0]
                    o["level"][k, i] = level
                    o["ambiguous"][k, i] = rule(fr["ratio"][i], lsf, levels)[1]
                    reached, bi, bd, nd = search_pair(kf, grid, fr, i, level, desc[i], th, counters)
                    o["raw_best_idx"][k, i], o["raw_best_dist"][k, i], o["n_dist"][k, i] = bi, bd, nd
                    if reached == CANDIDATE:
                        o["best_idx"][k, i], o["best_dist"][k, i] = bi, bd
            o["reached"][k, i] = reached
            if counters is not None:
                counters[REACHED[reached]] += 1
                counters["ambiguous"] += int(o["ambiguous"][k, i])
    return o
