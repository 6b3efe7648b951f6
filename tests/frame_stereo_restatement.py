"""numpy restatement of Frame::ComputeStereoLineMatches (reference src/Frame.cc:2008-2248) with
LineMatcher::SearchStereoMatchesByKnn (src/LineMatcher.cc:454-586) and ComputeDescriptorMatches (:2568-2620) inside it: one
match at a time in the reference's order, float32 where the reference computes in float, float64 where it builds
Eigen::Vector3d (cross by the plain formula, dot as c0 + (c1 + c2), v / s per component), with a counter per branch.
tests/golden/frame_stereo_reference.npz — the reference's own run (scripts/make_frame_stereo_golden.py) — pins it bit for
bit; the device code is held to the same file and, at other sizes, to this restatement."""
import numpy as np

f32, f64 = np.float32, np.float64

HISTO_LENGTH = 12
BRANCHES = ("ratio_test", "distance", "octave", "replaced", "equal_not_replaced", "rotation_bins_cut", "rotation_cut",
            "flag_matched_right", "octave_pm1", "vertical_span", "overlap", "ll0_small", "lr0_small", "lines_equal",
            "disparity_below", "disparity_above", "short_3d", "view_angle", "median_cut", "stereo")
_POP = np.array([bin(i).count("1") for i in range(256)], np.int64)


def knn2_mih(desc_q, desc_t):
    """Exact k = 2 neighbours of every query in the discovery order of the reference's multi-index hash (Mihasher(256, 32)): by
    distance, then the smallest per-byte distance s, the first byte k reaching it, the xor pattern of that byte, the train
    index.  -> idx [nq, 2], dist [nq, 2] (-1: absent) and the lowest-index neighbours for comparison."""
    nq, nt = len(desc_q), len(desc_t)
    idx, dist, low = -np.ones((nq, 2), np.int64), -np.ones((nq, 2), np.int64), -np.ones((nq, 2), np.int64)
    t = np.arange(nt, dtype=np.int64)
    for q in range(nq):
        x = np.bitwise_xor(desc_t, desc_q[q][None, :])
        pc = _POP[x]
        d, s, k = pc.sum(1), pc.min(1), pc.argmin(1)
        pat = x[t, k].astype(np.int64)
        key = (d << 48) | (s << 44) | (k.astype(np.int64) << 39) | (pat << 31) | t
        order = np.argsort(key, kind="stable")[:2]
        idx[q, :len(order)], dist[q, :len(order)] = order, d[order]
        lo = np.argsort((d << 32) | t, kind="stable")[:2]
        low[q, :len(lo)] = lo
    return idx, dist, low


def search_stereo_matches_by_knn(kl, desc, klr, desc_r, nn_ratio, check_orientation, descriptor_dist, counters):
    """-> vMatches as a list of [queryIdx, trainIdx, distance] and vValidMatches, in the reference's order."""
    idx, dist, _ = knn2_mih(desc, desc_r)
    two_pi = f32(2.0 * np.pi)                       # M_2PI, src/LineMatcher.cc:57
    factor = f32(HISTO_LENGTH) / two_pi
    nn_ratio = f32(nn_ratio)
    matches, slot_of, bin_of = [], {}, {}
    hist = [[] for _ in range(HISTO_LENGTH)]

    def rotation_bin(q, t):
        rot = f32(kl["angle"][q]) - f32(klr["angle"][t])
        if rot < 0.0:
            rot = f32(rot + two_pi)
        elif rot > two_pi:
            rot = f32(rot - two_pi)
        v = float(f32(rot * factor))                # round(): half away from zero (v + 0.5 is exact in double)
        b = int(np.floor(v + 0.5)) if v >= 0 else -int(np.floor(-v + 0.5))
        return 0 if b == HISTO_LENGTH else b

    for q in range(len(kl)):
        t = int(idx[q, 0])
        d0 = f32(dist[q, 0])
        if idx[q, 1] >= 0 and not (d0 < f32(nn_ratio * f32(dist[q, 1]))):
            counters["ratio_test"] += 1
            continue
        if not (d0 < descriptor_dist):
            counters["distance"] += 1
            continue
        if kl["octave"][q] != klr["octave"][t]:
            counters["octave"] += 1
            continue
        if t not in slot_of:
            matches.append([q, t, d0])
            slot_of[t] = len(matches) - 1
            if check_orientation:
                b = rotation_bin(q, t)
                hist[b].append(slot_of[t])
                bin_of[t] = b
        elif matches[slot_of[t]][2] > d0:
            counters["replaced"] += 1
            matches[slot_of[t]] = [q, t, d0]
            if check_orientation:
                hist[bin_of[t]].remove(slot_of[t])
                b = rotation_bin(q, t)
                hist[b].append(slot_of[t])
                bin_of[t] = b
        elif matches[slot_of[t]][2] == d0:
            counters["equal_not_replaced"] += 1
    valid = [True] * len(matches)
    if check_orientation:
        ind, mx = [-1, -1, -1], [0, 0, 0]
        for i in range(HISTO_LENGTH):               # ComputeThreeMaxima, :101-143
            s = len(hist[i])
            if s > mx[0]:
                mx, ind = [s, mx[0], mx[1]], [i, ind[0], ind[1]]
            elif s > mx[1]:
                mx, ind = [mx[0], s, mx[1]], [ind[0], i, ind[1]]
            elif s > mx[2]:
                mx[2], ind[2] = s, i
        if f32(mx[1]) < f32(0.1) * f32(mx[0]):
            ind[1] = ind[2] = -1
        elif f32(mx[2]) < f32(0.1) * f32(mx[0]):
            ind[2] = -1
        for i in range(HISTO_LENGTH):
            if i in ind:
                continue
            if hist[i]:
                counters["rotation_bins_cut"] += 1
            for slot in hist[i]:
                valid[slot] = False
                counters["rotation_cut"] += 1
    return matches, valid


def _cross(a, b):
    return [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]


def _dot(a, b):
    return a[0] * b[0] + (a[1] * b[1] + a[2] * b[2])


def _lines_equal(l1, l2, dot_threshold, dist_threshold):
    """Geom2DUtils::areLinesEqual (include/Geom2DUtils.h:162-180)"""
    normals_dot = f32(l1[0] * l2[0] + l1[1] * l2[1])
    d1, d2 = f32(l1[2]), f32(l2[2])
    if abs(f64(1.) - f64(abs(normals_dot))) < f64(dot_threshold):
        if normals_dot < 0:
            d1 = f32(d1 * f32(-1))
        if f32(abs(f32(d1 - d2))) < dist_threshold:
            return True
    return False


def _overlap(ys1, ye1, ys2, ye2):
    ymin1, ymax1, ymin2, ymax2 = min(ys1, ye1), max(ys1, ye1), min(ys2, ye2), max(ys2, ye2)
    if ymax2 < ymin1 or ymin2 > ymax1:
        return f64(0.)
    return min(ymax1, ymax2) - max(ymin1, ymin2)


def stereo_line_matches(kl, desc, klr, desc_r, sigma2, K4, mbf, line_stereo_max_dist, min_line_length_3d, nn_ratio=0.7,
                        check_orientation=True, descriptor_dist=50, counters=None, matcher=None):
    """-> (mvuRightLineStart, mvDepthLineStart, mvuRightLineEnd, mvDepthLineEnd, lines with depth).  kl / klr: key lines
    (structured arrays), desc / desc_r: [n, 32] uint8.  counters: filled per branch; matcher: a dict that receives vMatches /
    vValidMatches."""
    n = len(kl)
    counters = counters if counters is not None else {}
    for k in BRANCHES:
        counters[k] = 0
    out = [np.full(n, -1, f32) for _ in range(4)]
    if n == 0 or len(klr) == 0:
        return (*out, 0)
    K4 = np.asarray(K4, f32)
    mbf, fx, fy, cx, cy = f32(mbf), K4[0], K4[1], K4[2], K4[3]
    invfx, invfy = f32(1.0) / fx, f32(1.0) / fy
    mb = f32(mbf / fx)
    min_z, max_z = mb, min(mbf, f32(line_stereo_max_dist))
    min_d, max_d = f32(mbf / max_z), f32(mbf / min_z)
    cos_max = f32(np.cos(f64(30.) * f64(np.pi) / f64(f32(180.))))
    with np.errstate(all="ignore"):
        matches, valid = search_stereo_matches_by_knn(kl, desc, klr, desc_r, nn_ratio, check_orientation, descriptor_dist, counters)
        if matcher is not None:
            matcher["matches"], matcher["valid"] = [list(m) for m in matches], list(valid)
        flag_right = np.zeros(len(klr), bool)
        dist_idx = []
        for (q, t, dist), ok in zip(matches, valid):
            if not ok:
                continue
            if flag_right[t]:
                counters["flag_matched_right"] += 1
                continue
            sigma = f32(np.sqrt(f32(sigma2[kl["octave"][q]])))
            if klr["octave"][t] < kl["octave"][q] - 1 or klr["octave"][t] > kl["octave"][q] + 1:
                counters["octave_pm1"] += 1
                continue
            uS, vS, uE, vE = (f32(kl[k][q]) for k in ("startPointX", "startPointY", "endPointX", "endPointY"))
            ruS, rvS, ruE, rvE = (f32(klr[k][t]) for k in ("startPointX", "startPointY", "endPointX", "endPointY"))
            dyl, dyr = f32(abs(f32(vS - vE))), f32(abs(f32(rvS - rvE)))
            min_span = f32(f32(2) * sigma)
            if dyl <= min_span or dyr <= min_span:
                counters["vertical_span"] += 1
                continue
            if _overlap(f64(vS), f64(vE), f64(rvS), f64(rvE)) <= f64(f32(f32(2) * sigma)):
                counters["overlap"] += 1
                continue
            startL, endL = [f64(uS), f64(vS), f64(1.0)], [f64(uE), f64(vE), f64(1.0)]
            ll = _cross(startL, endL)
            s = np.sqrt(ll[0] * ll[0] + ll[1] * ll[1])
            ll = [ll[0] / s, ll[1] / s, ll[2] / s]
            lr = _cross([f64(ruS), f64(rvS), f64(1.0)], [f64(ruE), f64(rvE), f64(1.0)])
            s = np.sqrt(lr[0] * lr[0] + lr[1] * lr[1])
            lr = [lr[0] / s, lr[1] / s, lr[2] / s]
            dot_threshold, dist_threshold = f32(f32(0.005) * sigma), f32(f32(2) * sigma)
            if abs(ll[0]) < f64(dot_threshold):
                counters["ll0_small"] += 1
                continue
            if abs(lr[0]) < f64(dot_threshold):
                counters["lr0_small"] += 1
                continue
            if _lines_equal(ll, lr, dot_threshold, dist_threshold):
                counters["lines_equal"] += 1
                continue
            disparity_s, disparity_e = _dot(lr, startL) / lr[0], _dot(lr, endL) / lr[0]
            if not (disparity_s >= f64(min_d) and disparity_s <= f64(max_d) and disparity_e >= f64(min_d) and disparity_e <= f64(max_d)):
                counters["disparity_below" if (disparity_s < f64(min_d) or disparity_e < f64(min_d)) else "disparity_above"] += 1
                continue
            dS, dE = f32(f64(mbf) / disparity_s), f32(f64(mbf) / disparity_e)
            o = [f32(startL[0] - disparity_s), dS, f32(endL[0] - disparity_e), dE]
            if dS > 0 and dE > 0:
                xS, yS = f32(f32(f32(uS - cx) * dS) * invfx), f32(f32(f32(vS - cy) * dS) * invfy)
                xE, yE = f32(f32(f32(uE - cx) * dE) * invfx), f32(f32(f32(vE - cy) * dE) * invfy)
                ray = [f64(xS), f64(yS), f64(dS)]
                z2 = _dot(ray, ray)
                if z2 > 0:
                    r = np.sqrt(z2)
                    ray = [ray[0] / r, ray[1] / r, ray[2] / r]
                es = [f64(f32(xS - xE)), f64(f32(yS - yE)), f64(f32(dS - dE))]
                length = np.sqrt(_dot(es, es))
                if length < f64(f32(min_line_length_3d)):
                    counters["short_3d"] += 1
                    dS = dE = f32(-1)
                else:
                    es = [es[0] / length, es[1] / length, es[2] / length]
                    if f32(abs(f32(_dot(ray, es)))) > cos_max:
                        counters["view_angle"] += 1
                        dS = dE = f32(-1)
            if dS > 0 and dE > 0:
                flag_right[t] = True
                dist_idx.append((int(dist), q))
                for a, v in zip(out, o):
                    a[q] = v
        if dist_idx:
            dist_idx.sort()
            median = f32(dist_idx[len(dist_idx) // 2][0])
            th = f32(f32(f32(1.5) * f32(1.48)) * median)
            for first, q in reversed(dist_idx):
                if f32(first) < th:
                    break
                counters["median_cut"] += 1
                for a in out:
                    a[q] = f32(-1)
    counters["stereo"] = int((out[1] > 0).sum())
    return (*out, counters["stereo"])
