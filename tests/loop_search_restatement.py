"""numpy restatement of the loop-closing SearchByProjection overloads — ORBmatcher::SearchByProjection(pKF, Scw, vpPoints, vpMatched, th,
ratioHamming) (reference src/ORBmatcher.cc:509-615), the same with vpPointsKFs / vpMatchedKF (:617-730), and
LineMatcher::SearchByProjection(pKF, Scw, vpLines, vpMatched, th, ratioHamming) (src/LineMatcher.cc:1767-1909) with its vpLinesKFs /
vpMatchedKF overload (:1913-2037, the same search) — held bit for bit against the reference's compiled definitions by tests/test_loop_search.py (tests/golden/loop_search_reference.npz,
scripts/make_loop_search_golden.py) before any test relies on it at other sizes.

Up to the window both are the Sim3 Fuse's restatement (tests/loop_fuse_restatement.py, tests/orb_fuse_restatement.py) on the pose the
caller decomposed from Scw, except that the second overload projects by invz = 1 / z; u = fx * (x * invz) + cx (:657-662) where the
first calls Pinhole::project = fx * x / z + cx (:548).  Behind it they are GREEDY, and restated as the reference runs them: per key
frame a vpMatched array (seeded from `occupied`), the points in index order, per point the window's members in enumeration order with
`if(vpMatched[idx]) continue` first (:587), then the level band, then dist < bestDist from 256; bestDist <= TH_LOW * ratioHamming as
the f32 product it is (:606); vpMatched[bestIdx] = pMP.  The line overloads: the Sim3 line Fuse's front and window
(tests/line_fuse_restatement.py: ProjectLineWithCheck, Ow = -Rcw.transpose() * tcw, GetLineFeaturesInArea), then the same three
statements (:1863, :1868, :1894 with TH_LOW 60 and `&& (bestIdx >= 0)`).

`reached` as include/plvs_hip.h defines it for these entries: NO_CANDIDATE — nobody in the window passed the level band, claimed or
not; ABOVE_TH_LOW — no unclaimed member at or below the threshold."""
import numpy as np

from tests import line_fuse_restatement as LR
from tests import orb_fuse_restatement as PR
from tests.loop_fuse_restatement import line_kf, point_kf
from tests.track_local_restatement import predict_scale, rule
from tests.track_motion_restatement import se3_act

f32 = np.float32
_POP = PR._POP
CAMERA, INVZ = 0, 1
POINT_TH_LOW, LINE_TH_LOW = 50, 60
POINT_FACTS = LINE_FACTS = ("took_behind_a_claimed_best", "all_banded_claimed", "tie_winner_not_lowest_index", "occupied_would_have_won", "dist_at_cut",
               "dist_at_cut_plus_1", "claimed_skipped", "windows_over_list_len")
LIST_LEN = 4      # plvs_amd/csrc/loop_search_pair.hpp: kListLen


def cut_of(th_low, ratio):
    """The largest integer distance d with f32(d) <= f32(th_low) * f32(ratio)."""
    lim = f32(th_low) * f32(ratio)
    return max((d for d in range(257) if f32(d) <= lim), default=-1)


def front(kf, points, projection):
    """PR.front with the projection of the overload: the fields PR.search_pair and PR.window read."""
    fr = PR.front(kf, points)
    if projection == CAMERA:
        return fr
    pos = np.asarray(points["pos"], f32).reshape(-1, 3)
    K4, b = np.asarray(kf["K4"], f32), np.asarray(kf["bounds4"], f32)
    with np.errstate(all="ignore"):
        pc = se3_act(kf["q_cw"], kf["tcw"], pos).astype(f32)
        invz = f32(1.0) / pc[:, 2]
        x, y = pc[:, 0] * invz, pc[:, 1] * invz
        u, v = K4[0] * x + K4[2], K4[1] * y + K4[3]
        inside = (u >= b[0]) & (u < b[1]) & (v >= b[2]) & (v < b[3])
    # the tests behind the image test read neither u nor v: PR.front's own cascade over an unbounded image, this image test in front
    behind_it = PR.front(dict(kf, bounds4=np.array([-np.inf, np.inf, -np.inf, np.inf], f32)), points)["reached"]
    assert not (inside & (behind_it == PR.OUTSIDE)).any(), "a projection finite here and not in Pinhole::project"
    reached = np.where(fr["reached"] == PR.BEHIND, PR.BEHIND, np.where(inside, behind_it, PR.OUTSIDE)).astype(np.int32)
    return dict(fr, reached=reached, u=u.astype(f32), v=v.astype(f32))


def _pick(ind, octave, level, kdesc, desc, matched, entry, th_low, ratio, T, codes, counters, where):
    """The candidate loop and the decision behind it for a non-empty window `ind` (the reference's order) -> (reached, bestIdx, bestDist,
    distances taken); a match is written into `matched`."""
    no_candidate, above_th_low, candidate = codes
    band = (octave[ind] >= level - 1) & (octave[ind] <= level)
    free = ~matched[ind]
    cand = ind[free & band]            # if(vpMatched[idx]) continue first, then the level band
    best, best_idx = 256, -1
    d = np.zeros(0, np.int32)
    if len(cand):
        d = _POP[np.bitwise_xor(kdesc[cand], desc[None, :])].sum(1)
        j = int(np.argmin(d))          # dist < bestDist: the first minimum
        best, best_idx = int(d[j]), int(cand[j])
    if not band.any():
        reached = no_candidate
    elif f32(best) <= f32(th_low) * f32(ratio) and best_idx >= 0:
        reached = candidate
        matched[best_idx] = True
    else:
        reached = above_th_low
    if counters is not None and band.any():
        banded = ind[band]
        d_all = _POP[np.bitwise_xor(kdesc[banded], desc[None, :])].sum(1)
        jall = int(np.argmin(d_all))   # the winner had nobody been claimed
        note = lambda name: (counters.__setitem__(name, counters[name] + 1), counters["cases"].setdefault(name, list(where)))
        counters["claimed_skipped"] += int((~free & band).sum())
        if (d_all <= T).sum() > LIST_LEN:
            note("windows_over_list_len")
        if reached == candidate and matched[banded[jall]] and not entry[banded[jall]] and banded[jall] != best_idx:
            note("took_behind_a_claimed_best")
        if reached == candidate and entry[banded[jall]] and d_all[jall] <= T:
            note("occupied_would_have_won")
        if not len(cand):
            note("all_banded_claimed")
        if reached == candidate and (d == best).sum() > 1 and best_idx != cand[d == best].min():
            note("tie_winner_not_lowest_index")
        if reached == candidate and best == T:
            note("dist_at_cut")
        if reached == above_th_low and best == T + 1:
            note("dist_at_cut_plus_1")
    return reached, best_idx, best, len(cand)


def _seed(occupied, k, n):
    entry = np.zeros(n, bool)
    if occupied is not None and occupied[k] is not None:
        entry = np.asarray(occupied[k]).astype(bool).copy()
    return entry.copy(), entry


def point_search(kfs, points, skip, occupied, th, ratio, projection, counters=None, double_overload=False):
    """-> dict of [K, M] arrays: match_idx / match_dist (the entries' outputs), reached, raw_best_idx / raw_best_dist (bestIdx, bestDist as
    the loop left them: -1 / 256 without an unclaimed banded member), n_dist (Hamming distances taken), level, ambiguous, u, v, and
    nmatches [K]."""
    K, M = len(kfs), len(np.asarray(points["min_dist"]))
    T = cut_of(POINT_TH_LOW, ratio)
    o = dict(match_idx=np.full((K, M), -1, np.int32), match_dist=np.full((K, M), -1, np.int32), reached=np.zeros((K, M), np.uint8),
             raw_best_idx=np.full((K, M), -1, np.int32), raw_best_dist=np.full((K, M), 256, np.int32), n_dist=np.zeros((K, M), np.int32),
             level=np.full((K, M), -1, np.int32), ambiguous=np.zeros((K, M), np.uint8), u=np.zeros((K, M), f32), v=np.zeros((K, M), f32),
             nmatches=np.zeros(K, np.int32))
    if counters is not None:
        for k in PR.REACHED + POINT_FACTS + ("ambiguous",):
            counters.setdefault(k, 0)
        counters.setdefault("cases", {})
    desc = np.asarray(points["desc"], np.uint8).reshape(-1, 32)
    codes = (PR.NO_CANDIDATE, PR.ABOVE_TH_LOW, PR.CANDIDATE)
    for k, kf in enumerate(kfs):
        kf = point_kf(kf)
        grid = PR.grid_of(kf)
        fr = front(kf, points, projection)
        lsf, levels = f32(kf["log_scale_factor"]), len(kf["scale_factors"])
        matched, entry = _seed(occupied, k, len(kf["x"]))
        octave, kdesc = np.asarray(kf["octave"], np.int64), np.asarray(kf["desc"], np.uint8)
        for i in range(M):
            if skip is not None and skip[k][i]:
                reached = PR.SKIPPED
            else:
                reached = int(fr["reached"][i])
                if reached != PR.BEHIND:
                    o["u"][k, i], o["v"][k, i] = fr["u"][i], fr["v"][i]
                if reached == PR.EMPTY_WINDOW:
                    level = predict_scale(fr["ratio"][i], lsf, levels, double_overload)[0]
                    o["level"][k, i] = level
                    o["ambiguous"][k, i] = rule(fr["ratio"][i], lsf, levels)[1]
                    radius = f32(th) * np.asarray(kf["scale_factors"], f32)[level]
                    ind = PR.window(kf, grid, fr["u"][i], fr["v"][i], radius, None)
                    if len(ind):
                        reached, bi, bd, nd = _pick(ind, octave, level, kdesc, desc[i], matched, entry, POINT_TH_LOW, ratio, T, codes, counters, (k, i))
                        o["raw_best_idx"][k, i], o["raw_best_dist"][k, i], o["n_dist"][k, i] = bi, bd, nd
                        if reached == PR.CANDIDATE:
                            o["match_idx"][k, i], o["match_dist"][k, i] = bi, bd
                            o["nmatches"][k] += 1
            o["reached"][k, i] = reached
            if counters is not None:
                counters[PR.REACHED[reached]] += 1
                counters["ambiguous"] += int(o["ambiguous"][k, i])
    return o


def line_search(kfs, lines, skip, occupied, th, ratio, counters=None, log_double=False, atan_double=False):
    """-> dict of [K, M] arrays, the fields of point_search with proj [K, M, 6] / n_proj for u, v.  reached may be LR.FULL_THETA (the
    entries refuse the call)."""
    K, M = len(kfs), len(np.asarray(lines["max_dist"]))
    T = cut_of(LINE_TH_LOW, ratio)
    o = dict(match_idx=np.full((K, M), -1, np.int32), match_dist=np.full((K, M), -1, np.int32), reached=np.zeros((K, M), np.uint8),
             raw_best_idx=np.full((K, M), -1, np.int32), raw_best_dist=np.full((K, M), 256, np.int32), n_dist=np.zeros((K, M), np.int32),
             level=np.full((K, M), -1, np.int32), ambiguous=np.zeros((K, M), np.uint8), proj=np.zeros((K, M, 6), f32),
             n_proj=np.zeros((K, M), np.int32), nmatches=np.zeros(K, np.int32))
    if counters is not None:
        for k in LR.REACHED + LINE_FACTS + ("ambiguous_level", "ambiguous_theta"):
            counters.setdefault(k, 0)
        counters.setdefault("cases", {})
    desc = np.asarray(lines["desc"], np.uint8).reshape(-1, 32)
    codes = (LR.NO_CANDIDATE, LR.ABOVE_TH_LOW, LR.CANDIDATE)
    for k, kf in enumerate(kfs):
        kf = line_kf(kf)
        grid = LR.grid_of(kf, atan_double)
        fr = LR.front(kf, lines)
        lsf, levels = f32(kf["log_scale_factor"]), len(kf["scale_factors"])
        matched, entry = _seed(occupied, k, len(kf["kl"]))
        octave, kdesc = kf["kl"]["octave"].astype(np.int64), np.asarray(kf["desc"], np.uint8)
        for i in range(M):
            if skip is not None and skip[k][i]:
                reached = LR.SKIPPED
            else:
                reached = int(fr["reached"][i])
                n_proj = 0 if reached == LR.MIDDLE_BEHIND else (1 if reached < LR.END_OUTSIDE else (
                    2 if reached == LR.END_OUTSIDE and LR._outside(kf, fr["uS"][i], fr["vS"][i]) else 3))
                o["n_proj"][k, i] = n_proj
                o["proj"][k, i, :2 * n_proj] = [fr[c][i] for c in ("uM", "vM", "uS", "vS", "uE", "vE")][:2 * n_proj]
                if reached == LR.EMPTY_WINDOW:
                    level = predict_scale(fr["ratio"][i], lsf, levels, log_double)[0]
                    o["level"][k, i] = level
                    amb_level = rule(fr["ratio"][i], lsf, levels)[1]
                    nx, ny, d, n2 = LR.representation(fr["uS"][i], fr["vS"][i], fr["uE"][i], fr["vE"][i])
                    if n2 == 0:
                        reached = LR.DEGENERATE
                    else:
                        theta = LR.atan2_host(ny, nx, atan_double)
                        scale = np.asarray(kf["scale_factors"], f32)[level]
                        dtheta = f32(LR.K_DELTA_THETA * scale)
                        dd = f32(f32(f32(th) * LR.K_DELTA_D) * scale)
                        amb_theta = LR.theta_rule(ny, nx, dtheta)[1]
                        o["ambiguous"][k, i] = int(bool(amb_level or amb_theta))
                        if counters is not None:
                            counters["ambiguous_level"] += int(amb_level)
                            counters["ambiguous_theta"] += int(amb_theta)
                        ind, _ = LR.window(kf, grid, theta, d, dtheta, dd, None)
                        if ind is None:
                            reached = LR.FULL_THETA
                        elif len(ind):
                            reached, bi, bd, nd = _pick(ind, octave, level, kdesc, desc[i], matched, entry, LINE_TH_LOW, ratio, T, codes, counters,
                                                        (k, i))
                            o["raw_best_idx"][k, i], o["raw_best_dist"][k, i], o["n_dist"][k, i] = bi, bd, nd
                            if reached == LR.CANDIDATE:
                                o["match_idx"][k, i], o["match_dist"][k, i] = bi, bd
                                o["nmatches"][k] += 1
            o["reached"][k, i] = reached
            if counters is not None and reached < len(LR.REACHED):
                counters[LR.REACHED[reached]] += 1
    return o
