"""numpy restatement of the search stage of the two Sim3 Fuse overloads of LoopClosing::SearchAndFuse — ORBmatcher::Fuse(pKF, Scw,
vpPoints, th, vpReplacePoint) (reference src/ORBmatcher.cc:1437-1535) and LineMatcher::Fuse(pKF, Scw, vpLines, th, vpReplaceLine)
(src/LineMatcher.cc:2321-2530) — held bit for bit against the reference's compiled definitions by tests/test_loop_fuse.py
(tests/golden/loop_fuse_reference.npz, scripts/make_loop_fuse_golden.py) before any test relies on it at other sizes.

Both are the SE3 overloads' restatements (tests/orb_fuse_restatement.py, tests/line_fuse_restatement.py) up to the window — the same
projection, tests, PredictScale and GetFeaturesInArea / GetLineFeaturesInArea, on the pose the caller decomposed from Scw — with other
candidate gates:
  points  the level band [level - 1, level] alone (:1520); no chi-square gate, mvuRight is not read;
  lines   the level band, then the two point-to-line distances, squared, times mvLineInvLevelSigma2[nPredictedLevel] (:2463-2464) —
          not [klLevel] — against 3.84f; no right-image check (#if 0, :2471).
The line gate is restated by handing the SE3 restatement's search_pair a key frame whose mvLineInvLevelSigma2 holds the predicted
level's entry at every octave and whose mvuRightLineStart / End are empty: with them its text IS :2437-2467.

A key frame is the SE3 restatement's dict with the pose of include/plvs_hip.h's plvs_keyframe_sim3_pose: q_cw, Rcw, tcw, Ow_points,
Ow_lines (tests/loop_fuse_scenario.py also keeps scale and s_t = Scw.translation(), which only the maker's compiled run reads)."""
import numpy as np

from tests import line_fuse_restatement as LR
from tests import orb_fuse_restatement as PR
from tests.track_local_restatement import predict_scale, rule

f32 = np.float32
_POP = PR._POP
POINT_SUB_FACTS = ("dropped_below_level", "dropped_above_level", "clipped_left", "clipped_right", "clipped_top", "clipped_bottom",
                   "tie_winner_not_lowest_index", "dist3d_zero", "taken_outside_mono_chi2", "taken_outside_stereo_chi2")
LINE_SUB_FACTS = tuple(f for f in LR.SUB_FACTS if "right" not in f) + ("taken_where_kl_level_sigma_drops", "taken_where_right_gate_drops")


def point_kf(kf):
    """The key frame as the SE3 restatement's front() reads it: Ow = Tcw.inverse().translation()."""
    return dict(kf, Ow=kf["Ow_points"])


def line_kf(kf):
    """The same for the line side: Ow = -Rcw.transpose() * tcw."""
    return dict(kf, Ow=kf["Ow_lines"])


def point_search_pair(kf, grid, fr, i, level, desc, th, counters=None):
    """:1502-1535 for point i of `fr` = PR.front(...) -> (reached, bestIdx, bestDist, candidates whose distance was taken)."""
    radius = f32(th) * np.asarray(kf["scale_factors"], f32)[level]
    ind = PR.window(kf, grid, fr["u"][i], fr["v"][i], radius, counters)
    if len(ind) == 0:
        return PR.EMPTY_WINDOW, -1, 256, 0
    oct_ = np.asarray(kf["octave"], np.int64)[ind]
    below, above = oct_ < level - 1, oct_ > level
    cand = ind[~(below | above)]
    if counters is not None:
        counters["dropped_below_level"] += int(below.sum())
        counters["dropped_above_level"] += int(above.sum())
    if len(cand) == 0:
        return PR.NO_CANDIDATE, -1, 256, 0
    d = _POP[np.bitwise_xor(np.asarray(kf["desc"], np.uint8)[cand], np.asarray(desc, np.uint8)[None, :])].sum(1)
    j = int(np.argmin(d))            # the first minimum
    best, best_idx = int(d[j]), int(cand[j])
    if counters is not None and best <= PR.TH_LOW:
        if (d == best).sum() > 1 and best_idx != cand[d == best].min():
            counters["tie_winner_not_lowest_index"] += 1
        # what the SE3 overload's gate (:1365-1392) would have said of the winner
        with np.errstate(all="ignore"):
            ex, ey = fr["u"][i] - np.asarray(kf["x"], f32)[best_idx], fr["v"][i] - np.asarray(kf["y"], f32)[best_idx]
            kr = np.asarray(kf["u_right"], f32)[best_idx]
            sig = np.asarray(kf["inv_level_sigma2"], f32)[oct_[~(below | above)][j]]
            er = fr["ur"][i] - kr
            if kr >= 0:
                counters["taken_outside_stereo_chi2"] += int(float(((ex * ex + ey * ey) + er * er) * sig) > 7.8)
            else:
                counters["taken_outside_mono_chi2"] += int(float((ex * ex + ey * ey) * sig) > 5.99)
    return (PR.CANDIDATE if best <= PR.TH_LOW else PR.ABOVE_TH_LOW), best_idx, best, len(cand)


def point_search(kfs, points, skip, th, counters=None, double_overload=False):
    """-> dict of [K, M] arrays, the fields of orb_fuse_restatement.fuse_search."""
    K, M = len(kfs), len(np.asarray(points["min_dist"]))
    o = dict(best_idx=np.full((K, M), -1, np.int32), best_dist=np.full((K, M), -1, np.int32), reached=np.zeros((K, M), np.uint8),
             raw_best_idx=np.full((K, M), -1, np.int32), raw_best_dist=np.full((K, M), 256, np.int32), n_dist=np.zeros((K, M), np.int32),
             level=np.full((K, M), -1, np.int32), ambiguous=np.zeros((K, M), np.uint8), u=np.zeros((K, M), f32), v=np.zeros((K, M), f32))
    if counters is not None:
        for k in PR.REACHED + POINT_SUB_FACTS + ("ambiguous",):
            counters.setdefault(k, 0)
    desc = np.asarray(points["desc"], np.uint8).reshape(-1, 32)
    for k, kf in enumerate(kfs):
        kf = point_kf(kf)
        grid = PR.grid_of(kf)
        fr = PR.front(kf, points)
        lsf, levels = f32(kf["log_scale_factor"]), len(kf["scale_factors"])
        for i in range(M):
            if skip is not None and skip[k][i]:
                reached = PR.SKIPPED
            else:
                reached = int(fr["reached"][i])
                if reached != PR.BEHIND:
                    o["u"][k, i], o["v"][k, i] = fr["u"][i], fr["v"][i]
                if counters is not None and reached == PR.VIEW_ANGLE and fr["dist_zero"][i]:
                    counters["dist3d_zero"] += 1
                if reached == PR.EMPTY_WINDOW:
                    level = predict_scale(fr["ratio"][i], lsf, levels, double_overload)[0]
                    o["level"][k, i] = level
                    o["ambiguous"][k, i] = rule(fr["ratio"][i], lsf, levels)[1]
                    reached, bi, bd, nd = point_search_pair(kf, grid, fr, i, level, desc[i], th, counters)
                    o["raw_best_idx"][k, i], o["raw_best_dist"][k, i], o["n_dist"][k, i] = bi, bd, nd
                    if reached == PR.CANDIDATE:
                        o["best_idx"][k, i], o["best_dist"][k, i] = bi, bd
            o["reached"][k, i] = reached
            if counters is not None:
                counters[PR.REACHED[reached]] += 1
                counters["ambiguous"] += int(o["ambiguous"][k, i])
    return o


def _sim3_gate_kf(kf, level):
    """The key frame with which LR.search_pair's gate is :2437-2467 for a pair predicted at `level` (see the head)."""
    sig = np.asarray(kf["inv_level_sigma2"], f32)
    return dict(kf, inv_level_sigma2=np.full(len(sig), sig[level], f32), u_right_start=None, u_right_end=None)


def line_search(kfs, lines, skip, th, counters=None, log_double=False, atan_double=False):
    """-> dict of [K, M] arrays, the fields of line_fuse_restatement.fuse_search."""
    K, M = len(kfs), len(np.asarray(lines["max_dist"]))
    o = dict(best_idx=np.full((K, M), -1, np.int32), best_dist=np.full((K, M), -1, np.int32), reached=np.zeros((K, M), np.uint8),
             raw_best_idx=np.full((K, M), -1, np.int32), raw_best_dist=np.full((K, M), 256, np.int32), n_dist=np.zeros((K, M), np.int32),
             level=np.full((K, M), -1, np.int32), ambiguous=np.zeros((K, M), np.uint8), proj=np.zeros((K, M, 6), f32),
             n_proj=np.zeros((K, M), np.int32))
    if counters is not None:
        for k in LR.REACHED + LR.SUB_FACTS + LINE_SUB_FACTS + ("ambiguous_level", "ambiguous_theta"):
            counters.setdefault(k, 0)
    desc = np.asarray(lines["desc"], np.uint8).reshape(-1, 32)
    for k, kf in enumerate(kfs):
        kf = line_kf(kf)
        grid = LR.grid_of(kf, atan_double)
        fr = LR.front(kf, lines)
        lsf, levels = f32(kf["log_scale_factor"]), len(kf["scale_factors"])
        gate_kf = [_sim3_gate_kf(kf, lv) for lv in range(levels)]
        for i in range(M):
            if skip is not None and skip[k][i]:
                reached = LR.SKIPPED
            else:
                reached = int(fr["reached"][i])
                n_proj = 0 if reached == LR.MIDDLE_BEHIND else (1 if reached < LR.END_OUTSIDE else (
                    2 if reached == LR.END_OUTSIDE and LR._outside(kf, fr["uS"][i], fr["vS"][i]) else 3))
                o["n_proj"][k, i] = n_proj
                o["proj"][k, i, :2 * n_proj] = [fr[c][i] for c in ("uM", "vM", "uS", "vS", "uE", "vE")][:2 * n_proj]
                if counters is not None and reached == LR.DEGENERATE:
                    counters["dist_zero"] += 1
                if reached == LR.EMPTY_WINDOW:
                    level = predict_scale(fr["ratio"][i], lsf, levels, log_double)[0]
                    o["level"][k, i] = level
                    amb_level = rule(fr["ratio"][i], lsf, levels)[1]
                    reached, bi, bd, nd, amb_theta = LR.search_pair(gate_kf[level], grid, fr, i, level, desc[i], th, counters, atan_double)
                    o["ambiguous"][k, i] = int(bool(amb_level or amb_theta))
                    o["raw_best_idx"][k, i], o["raw_best_dist"][k, i], o["n_dist"][k, i] = bi, bd, nd
                    if reached == LR.CANDIDATE:
                        o["best_idx"][k, i], o["best_dist"][k, i] = bi, bd
                    if counters is not None:
                        counters["ambiguous_level"] += int(amb_level)
                        counters["ambiguous_theta"] += int(amb_theta)
                        if reached == LR.CANDIDATE and not amb_theta:
                            # what the SE3 overload's gates (:2198-2250) would have said of the same pair
                            se3 = LR.search_pair(kf, grid, fr, i, level, desc[i], th, None, atan_double)
                            no_right = LR.search_pair(dict(kf, u_right_start=None, u_right_end=None), grid, fr, i, level, desc[i], th, None,
                                                      atan_double)
                            counters["taken_where_kl_level_sigma_drops"] += int(no_right[1] != bi)
                            counters["taken_where_right_gate_drops"] += int(no_right[1] == bi and se3[1] != bi)
            o["reached"][k, i] = reached
            if counters is not None and reached < len(LR.REACHED):
                counters[LR.REACHED[reached]] += 1
    return o
