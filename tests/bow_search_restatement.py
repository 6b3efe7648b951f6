"""ORBmatcher::SearchByBoW(pKF1, pKF2, vpMatches12) (reference src/ORBmatcher.cc:853-997) and SearchByBoW(pKF, F, vpMapPointMatches)
(:300-507) restated in numpy for single-camera frames, statement by statement, with what the compiled reference does not hand out:
bestDist1 / bestDist2 and the raw best of every serial feature, the bin of every match, and counters of the placed cases.
scripts/make_bow_search_golden.py pins this file to the compiled reference cuts bit for bit.

A side: tests/bow_search_scenario.py's dict.  serial: the side the reference walks in its outer loop (KF1; KF), lane: the other (KF2; F)."""
import math

import numpy as np

TH_LOW = 50          # ORBmatcher::TH_LOW, :58
HISTO_LENGTH = 12    # :61
KF, FRAME = "kf", "frame"
_POP = np.array([bin(i).count("1") for i in range(256)], np.int32)


def distances(q, members):
    """DescriptorDistance (:2198-2225) of one descriptor to each of `members` [m,32]."""
    return _POP[np.bitwise_xor(members, q[None, :])].sum(axis=1).astype(np.int32)


def three_maxima(counts):
    """ComputeThreeMaxima (:2123-2164) on bin counts."""
    max1 = max2 = max3 = 0
    ind1 = ind2 = ind3 = -1
    for i, s in enumerate(counts):
        if s > max1:
            max3, max2, max1 = max2, max1, s
            ind3, ind2, ind1 = ind2, ind1, i
        elif s > max2:
            max3, max2 = max2, s
            ind3, ind2 = ind2, i
        elif s > max3:
            max3, ind3 = s, i
    if np.float32(max2) < np.float32(0.1) * np.float32(max1):
        ind2 = ind3 = -1
    elif np.float32(max3) < np.float32(0.1) * np.float32(max1):
        ind3 = -1
    return ind1, ind2, ind3


def rotation_bin(angle_serial, angle_lane):
    """:949-954 / :426-431: f32 throughout, round half away from zero, bin 12 -> 0.  -> (bin, the rounded value before the wrap)."""
    rot = np.float32(angle_serial) - np.float32(angle_lane)
    if rot < 0.0:
        rot = np.float32(rot + np.float32(360.0))
    x = np.float32(rot * (np.float32(HISTO_LENGTH) / np.float32(360.0)))
    raw = int(math.floor(float(x) + 0.5))
    return (0 if raw == HISTO_LENGTH else raw), raw


def search(serial, lane, kind, nn_ratio, check_orientation, counts=None):
    """-> dict(match [n_out]: kf kind — per serial feature the lane feature matched; frame kind — per lane (frame) feature the serial
    (key-frame) feature assigned; match_dist [n_out]; nmatches; per SERIAL feature: best1, best2 (-1: not evaluated), raw_idx (the
    lane feature of bestDist1, -1 none), n_dist, raw_bin (the rounded rot * factor of an accepted match, else -1), cut (1: accepted,
    then removed by the rotation check))."""
    ns, nl = len(serial["desc"]), len(lane["desc"])
    s_valid = serial["ref_valid"] == 1
    l_open = np.ones(nl, bool) if kind == FRAME else (lane["ref_valid"] == 1)     # :918-922 / :359
    claimed = np.zeros(nl, bool)
    n_out = nl if kind == FRAME else ns
    match = np.full(n_out, -1, np.int32)
    match_dist = np.full(n_out, -1, np.int32)
    best1, best2 = np.full(ns, -1, np.int32), np.full(ns, -1, np.int32)
    raw_idx, n_dist, raw_bin, cut = np.full(ns, -1, np.int32), np.zeros(ns, np.int32), np.full(ns, -1, np.int32), np.zeros(ns, np.uint8)
    c = counts if counts is not None else {}
    for key in ("common_nodes", "multi_pass_jobs", "best2_stays_256", "best1_stays_256_all_closed", "equal_minima", "tie_winner_not_lowest_index",
                "took_behind_a_closed_best", "best1_at_th_low", "best1_at_th_low_accepted", "ratio_at_equality", "bin_12", "bin_tie_at_cut",
                "serial_list_of_1", "cut_by_rotation", "accepted"):
        c.setdefault(key, 0)
    c.setdefault("lane_lengths", [])
    hist = [[] for _ in range(HISTO_LENGTH)]
    nmatches = 0
    nn = np.float32(nn_ratio)
    for node, s_list in serial["nodes"].items():          # the intersection of the two ascending id lists
        if node not in lane["nodes"]:
            continue
        l_list = np.asarray(lane["nodes"][node], np.int64)
        c["common_nodes"] += 1
        c["multi_pass_jobs"] += len(l_list) > 64
        evaluated = False
        for i_s in s_list:
            if not s_valid[i_s]:
                continue
            evaluated = True
            open_ = l_open[l_list] & ~claimed[l_list]
            d_all = distances(serial["desc"][i_s], lane["desc"][l_list]) if len(l_list) else np.zeros(0, np.int32)
            b1, b2, bi = 256, 256, -1
            for q in np.flatnonzero(open_):
                d = int(d_all[q])
                if d < b1:
                    b2, b1, bi = b1, d, int(l_list[q])
                elif d < b2:
                    b2 = d
            n_dist[i_s] = int(open_.sum())
            best1[i_s], best2[i_s], raw_idx[i_s] = b1, b2, bi
            # ---- the placed cases
            if open_.any() and b2 == 256 and b1 < 256:
                c["best2_stays_256"] += 1
            if len(l_list) and not open_.any():
                c["best1_stays_256_all_closed"] += 1
            if b1 == b2 and b1 < 256:
                c["equal_minima"] += 1
            if bi >= 0 and (d_all[open_] == b1).sum() > 1 and bi > l_list[open_][d_all[open_] == b1].min():
                c["tie_winner_not_lowest_index"] += 1
            closed_d = d_all[~open_ & claimed[l_list]]
            if bi >= 0 and len(closed_d) and closed_d.min() < b1:
                c["took_behind_a_closed_best"] += 1
            if b1 == TH_LOW:
                c["best1_at_th_low"] += 1
            if np.float32(b1) == nn * np.float32(b2):
                c["ratio_at_equality"] += 1
            if (b1 <= TH_LOW if kind == FRAME else b1 < TH_LOW) and np.float32(b1) < nn * np.float32(b2):     # :940-942 / :408-410
                c["accepted"] += 1
                if b1 == TH_LOW:
                    c["best1_at_th_low_accepted"] += 1
                claimed[bi] = True
                at = bi if kind == FRAME else i_s
                match[at] = i_s if kind == FRAME else bi
                match_dist[at] = b1
                if check_orientation:
                    b, raw = rotation_bin(serial["angle"][i_s], lane["angle"][bi])
                    raw_bin[i_s] = raw
                    c["bin_12"] += raw == HISTO_LENGTH
                    hist[b].append((at, i_s))
                nmatches += 1
        if evaluated:
            c["lane_lengths"].append(len(l_list))
            c["serial_list_of_1"] += len(s_list) == 1
    if check_orientation:
        sizes = [len(h) for h in hist]
        ind = three_maxima(sizes)
        kept = [sizes[i] for i in ind if i >= 0]
        if kept and any(sizes[i] == min(kept) and sizes[i] > 0 for i in range(HISTO_LENGTH) if i not in ind):
            c["bin_tie_at_cut"] += 1
        for i in range(HISTO_LENGTH):
            if i in ind:
                continue
            for at, i_s in hist[i]:
                match[at] = match_dist[at] = -1
                cut[i_s] = 1
                c["cut_by_rotation"] += 1
                nmatches -= 1
    c["lane_lengths"] = sorted(set(c["lane_lengths"]))
    return dict(match=match, match_dist=match_dist, nmatches=nmatches, best1=best1, best2=best2, raw_idx=raw_idx, n_dist=n_dist, raw_bin=raw_bin,
                cut=cut)


def search_call(a_side, b_sides, kind, nn_ratio, check_orientation, counts=None):
    """One library call: kf kind — SearchByBoW(A, B[k]); frame kind — SearchByBoW(B[k], F = A).  -> (match [K,n_A], match_dist [K,n_A],
    nmatches [K], the per-k dicts)."""
    per_k = [search(a_side, b, KF, nn_ratio, check_orientation, counts) if kind == KF else search(b, a_side, FRAME, nn_ratio, check_orientation, counts)
             for b in b_sides]
    n = len(a_side["desc"])
    match = np.array([r["match"] for r in per_k], np.int32).reshape(len(b_sides), n)
    dist = np.array([r["match_dist"] for r in per_k], np.int32).reshape(len(b_sides), n)
    return match, dist, np.array([r["nmatches"] for r in per_k], np.int32), per_k
