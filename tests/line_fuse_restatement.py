"""numpy restatement of the search stage of LineMatcher::Fuse(pKF, vpMapLines, th, bRight = false) (reference
src/LineMatcher.cc:2043-2276), held bit for bit against the reference's compiled definitions by tests/test_line_fuse.py
(tests/golden/line_fuse_reference.npz, scripts/make_line_fuse_golden.py) before any test relies on it at other sizes.

Per pair: LineProjection::ProjectLineWithCheck for a pinhole camera in its own order (include/LineProjection.h:144-264: the middle
point as an f32 halving, R p + t with the product first, projectLinear, four comparisons a NaN passes, the CAMERA-frame norm
sqrt(c0 + (c1 + c2)), the band 0.8f / 1.2f * mfMaxDistance, both depths before either projection, invSz = 1.0f / z), PO = p3DMw - Ow
with the WORLD middle point, PO.dot(Pn) < 0.5 * distMiddlePoint compared in f64, MapLine::PredictScale through the C library's logf,
Geom2DUtils::GetLine2dRepresentation through the C library's atan2f, KeyFrame::GetLineFeaturesInArea (src/KeyFrame.cc:1291-1402:
the rows in f64, the columns in f32 with the key frame's int mnMaxDiag, the split at +-pi/2 with the wrapped sub-window first), the
level band, the point-to-line gates compared in f32 against 3.84f, the right-image gates, the first minimum in enumeration order.
Every operation is one f32 numpy operation: no contraction.

A key frame is a dict(kl (KEYLINE_DTYPE), desc, u_right_start, u_right_end (None: empty), mbf, scale_factors, inv_level_sigma2,
max_diag (the Frame's float mnMaxDiag), log_scale_factor, K4, bounds4, Rcw (9, column-major), tcw, Ow); lines a dict(start, end,
normal, max_dist, desc)."""
import ctypes
import ctypes.util
import math

import numpy as np

from tests.track_local_restatement import _cam, _norm, _project, predict_scale, rule

f32 = np.float32
REACHED = ("skipped", "middle_behind", "middle_outside", "too_near", "too_far", "end_behind", "end_outside", "view_angle", "degenerate",
           "empty_window", "no_candidate", "above_th_low", "candidate")
(SKIPPED, MIDDLE_BEHIND, MIDDLE_OUTSIDE, TOO_NEAR, TOO_FAR, END_BEHIND, END_OUTSIDE, VIEW_ANGLE, DEGENERATE, EMPTY_WINDOW, NO_CANDIDATE,
 ABOVE_TH_LOW, CANDIDATE) = range(13)
FULL_THETA = 13           # fabs(thetaMin - thetaMax) > M_PI: the reference leaves the process, the entries refuse the call
ROWS, COLS, TH_LOW = 36, 160, 60
THETA_ULPS = 4            # line_fuse_pair.hpp: kThetaUlps
SUB_FACTS = ("dropped_below_level", "dropped_above_level", "dropped_start_gate_alone", "dropped_end_gate_alone", "dropped_right_gate_alone",
             "u_right_start_zero_stereo_branch", "u_right_end_negative_skips_stereo", "u_right_empty", "split_at_minus_half_pi",
             "split_at_plus_half_pi", "split_members_on_both_sides", "clipped_column_0", "clipped_column_159", "window_misses_grid",
             "tie_winner_in_wrapped_part_higher_index", "best_dist_60", "best_dist_61", "beyond_member_64", "dist_zero",
             "end_points_coincide")
_POP = np.array([bin(i).count("1") for i in range(256)], np.int32)
EPS = f32(1.1920929e-07)
CHI2 = f32(3.84)
K_DELTA_THETA = f32(10 * math.pi / float(f32(180.0)))     # Frame::kDeltaTheta = 10 * M_PI / 180.f, a const float
K_DELTA_D = f32(100)
THETA_INV = f32(ROWS) / f32(math.pi)                      # mfLineGridElementThetaInv

_libm = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
_libm.atan2f.restype = ctypes.c_float
_libm.atan2f.argtypes = [ctypes.c_float, ctypes.c_float]
_libm.atan2.restype = ctypes.c_double
_libm.atan2.argtypes = [ctypes.c_double, ctypes.c_double]


def atan2_host(ny, nx, double_overload=False):
    """theta of GetLine2dRepresentation on the C library: atan2f (what the compiled reference calls), or atan2 rounded to f32."""
    return f32(_libm.atan2(float(ny), float(nx))) if double_overload else f32(_libm.atan2f(float(ny), float(nx)))


def _c_round(v):
    """C round(): half away from zero."""
    v = float(v)
    return math.floor(v + 0.5) if v >= 0 else math.ceil(v - 0.5)


def representation(xs, ys, xe, ye):
    """GetLine2dRepresentationNoTheta -> (nx, ny, d, n2) in f32; n2 == 0: the normal is 0 * inf."""
    xs, ys, xe, ye = f32(xs), f32(ys), f32(xe), f32(ye)
    with np.errstate(all="ignore"):
        nx, ny = f32(ye - ys), f32(xs - xe)
        if nx < 0:
            nx, ny = f32(nx * f32(-1.0)), f32(ny * f32(-1.0))
        n2 = f32(f32(nx * nx) + f32(ny * ny))
        inv = f32(f32(1.0) / np.sqrt(n2))
        nx, ny = f32(nx * inv), f32(ny * inv)
        d = f32(f32(nx * xe) + f32(ny * ye))
    return nx, ny, d, n2


def d_inv_of(kf):
    return f32(f32(COLS) / f32(f32(2.0) * f32(kf["max_diag"])))        # mfLineGridElementDInv, from the Frame's float diagonal


def grid_of(kf, double_overload=False):
    """Frame::PosLineInGrid (src/Frame.cc:1477-1495), which the key frame copies: cells in (column, row) order as starts + members in
    insertion order; a key line outside the grid is in no cell."""
    kl = kf["kl"]
    dinv, diag = d_inv_of(kf), f32(kf["max_diag"])
    cell = np.full(len(kl), -1, np.int64)
    for i in range(len(kl)):
        nx, ny, d, _ = representation(kl["startPointX"][i], kl["startPointY"][i], kl["endPointX"][i], kl["endPointY"][i])
        theta = atan2_host(ny, nx, double_overload)
        if not (math.isfinite(float(theta)) and math.isfinite(float(d))):
            continue
        row = _c_round((float(theta) + math.pi / 2) * float(THETA_INV))
        col = _c_round(f32(f32(d + diag) * dinv))
        if 0 <= row < ROWS and 0 <= col < COLS:
            cell[i] = int(col) * ROWS + int(row)
    idx = np.flatnonzero(cell >= 0)
    order = idx[np.argsort(cell[idx], kind="stable")]
    start = np.zeros(COLS * ROWS + 1, np.int64)
    np.add.at(start, cell[idx] + 1, 1)
    return np.cumsum(start), order


def front(kf, lines):
    """ProjectLineWithCheck and :2103-2116 over all lines -> dict(reached (a rejection, or EMPTY_WINDOW = every test passed), uS, vS, uE,
    vE, invSz, invEz, dist, ratio, dist_zero)."""
    S, E = np.asarray(lines["start"], f32).reshape(-1, 3), np.asarray(lines["end"], f32).reshape(-1, 3)
    nrm, maxd = np.asarray(lines["normal"], f32).reshape(-1, 3), np.asarray(lines["max_dist"], f32)
    b, Ow, K4 = np.asarray(kf["bounds4"], f32), np.asarray(kf["Ow"], f32), kf["K4"]
    with np.errstate(all="ignore"):
        Mw = ((S + E) * f32(0.5)).astype(f32)
        Mc, Sc, Ec = _cam(kf["Rcw"], kf["tcw"], Mw), _cam(kf["Rcw"], kf["tcw"], S), _cam(kf["Rcw"], kf["tcw"], E)
        out = lambda u, v: (u < b[0]) | (u > b[1]) | (v < b[2]) | (v > b[3])
        uM, vM = _project(K4, Mc)
        dist = _norm(Mc)
        uS, vS = _project(K4, Sc)
        uE, vE = _project(K4, Ec)
        invSz, invEz = (f32(1.0) / Sc[:, 2]).astype(f32), (f32(1.0) / Ec[:, 2]).astype(f32)
        PO = Mw - Ow[None, :]
        dot = PO[:, 0] * nrm[:, 0] + (PO[:, 1] * nrm[:, 1] + PO[:, 2] * nrm[:, 2])
        ratio = (maxd / dist).astype(f32)
        order = ((dist == 0, DEGENERATE), (dot.astype(np.float64) < 0.5 * dist.astype(np.float64), VIEW_ANGLE),
                 (out(uS, vS) | out(uE, vE), END_OUTSIDE), ((Sc[:, 2] < 0) | (Ec[:, 2] < 0), END_BEHIND), (dist > f32(1.2) * maxd, TOO_FAR),
                 (dist < f32(0.8) * maxd, TOO_NEAR), (out(uM, vM), MIDDLE_OUTSIDE), (Mc[:, 2] < 0, MIDDLE_BEHIND))
    reached = np.full(len(S), EMPTY_WINDOW, np.int32)
    for mask, code in order:                 # the earliest test is written last
        reached[mask] = code
    return dict(reached=reached, uM=uM, vM=vM, uS=uS, vS=vS, uE=uE, vE=vE, invSz=invSz, invEz=invEz, dist=dist, ratio=ratio, dist_zero=(dist == 0))


def _floor_cell(v):
    v = float(v)
    return -1 if not v > -1.0 else (10 ** 6 if v > 1e6 else int(math.floor(v)))


def leaves(tmin, tmax, dmin, dmax, out, tags=None, tag="plain"):
    """KeyFrame::GetLineFeaturesInArea(thetaMin, thetaMax, dMin, dMax, ...) as it recurses (:1314-1357) -> the leaves in its order."""
    tmin, tmax, dmin, dmax = f32(tmin), f32(tmax), f32(dmin), f32(dmax)
    if len(out) > 8:
        return
    if float(tmin) < -math.pi / 2:
        leaves(f32(float(tmin) + math.pi), f32(math.pi / 2 - float(EPS)), f32(-dmax), f32(-dmin), out, tags, "wrapped_minus")
        leaves(f32(-math.pi / 2 + float(EPS)), tmax, dmin, dmax, out, tags, "rest_minus")
        return
    if float(tmax) > math.pi / 2:
        leaves(f32(-math.pi / 2 + float(EPS)), f32(float(tmax) - math.pi), f32(-dmax), f32(-dmin), out, tags, "wrapped_plus")
        leaves(tmin, f32(math.pi / 2 - float(EPS)), dmin, dmax, out, tags, "rest_plus")
        return
    out.append((tmin, tmax, dmin, dmax))
    if tags is not None:
        tags.append(tag)


def leaf_cells(kf, leaf):
    """:1362-1382 -> (r0, r1, c0, c1, raw c0, raw c1) or None (an early return)."""
    tmin, tmax, dmin, dmax = leaf
    diag, dinv = f32(int(f32(kf["max_diag"]))), d_inv_of(kf)          # KeyFrame::mnMaxDiag is an int
    r0 = max(0, _floor_cell((float(tmin) + math.pi / 2) * float(THETA_INV)))
    if r0 >= ROWS:
        return None
    r1 = min(ROWS - 1, _floor_cell((float(tmax) + math.pi / 2) * float(THETA_INV)))
    if r1 < 0:
        return None
    with np.errstate(all="ignore"):
        raw0, raw1 = _floor_cell(f32(f32(dmin + diag) * dinv)), _floor_cell(f32(f32(dmax + diag) * dinv))
    c0 = max(0, raw0)
    if c0 >= COLS:
        return None
    c1 = min(COLS - 1, raw1)
    if c1 < 0:
        return None
    return r0, r1, c0, c1, raw0, raw1


def window(kf, grid, theta, d, dtheta, dd, counters=None):
    """KeyFrame::GetLineFeaturesInArea(lineRepresentation, dtheta, dd) -> the indices in the reference's order (None: the interval is
    wider than pi), and per index whether it came from a wrapped sub-window."""
    start, order = grid
    tmin, tmax = f32(theta - dtheta), f32(theta + dtheta)
    if abs(float(f32(tmin - tmax))) > math.pi:
        return None, None
    out, tags = [], []
    leaves(tmin, tmax, f32(d - dd), f32(d + dd), out, tags)
    parts, wrapped, missed = [], [], True
    for leaf, tag in zip(out, tags):
        c = leaf_cells(kf, leaf)
        if c is None:
            continue
        missed = False
        r0, r1, c0, c1, raw0, raw1 = c
        if counters is not None:
            counters["clipped_column_0"] += raw0 < 0
            counters["clipped_column_159"] += raw1 > COLS - 1
        for ix in range(c0, c1 + 1):
            a, e = start[ix * ROWS + r0], start[ix * ROWS + r1 + 1]
            if e > a:
                parts.append(order[a:e])
                wrapped.append(np.full(e - a, tag.startswith("wrapped")))
    mem = np.concatenate(parts) if parts else np.zeros(0, np.int64)
    wr = np.concatenate(wrapped) if wrapped else np.zeros(0, bool)
    if counters is not None:
        counters["window_misses_grid"] += missed
        if "wrapped_minus" in tags:
            counters["split_at_minus_half_pi"] += 1
        if "wrapped_plus" in tags:
            counters["split_at_plus_half_pi"] += 1
        if len(wr) and wr.any() and not wr.all():
            counters["split_members_on_both_sides"] += 1
    return mem, wr


def theta_decisions(theta, dtheta):
    """What theta decides (line_fuse_pair.hpp: theta_plan): the refusal, the branch, the rows of every leaf."""
    tmin, tmax = f32(theta - dtheta), f32(theta + dtheta)
    if abs(float(f32(tmin - tmax))) > math.pi:
        return ("full",)
    out, tags = [], []
    leaves(tmin, tmax, f32(0), f32(0), out, tags)
    rows = []
    for tmin_, tmax_, _, _ in out:
        r0 = max(0, _floor_cell((float(tmin_) + math.pi / 2) * float(THETA_INV)))
        r1 = min(ROWS - 1, _floor_cell((float(tmax_) + math.pi / 2) * float(THETA_INV)))
        rows.append((min(r0, ROWS), max(r1, -1), r0 < ROWS and r1 >= 0))
    return tuple(tags), tuple(rows)


def theta_rule(ny, nx, dtheta):
    """The kernel's rule -> (theta_d = the f64 arctangent rounded to f32, ambiguous)."""
    theta = f32(math.atan2(float(ny), float(nx)))
    own = theta_decisions(theta, dtheta)
    amb = len(own) == 2 and len(own[0]) > 2          # a third sub-window: the host's recursion takes the pair
    t_lo = t_hi = theta
    for _ in range(THETA_ULPS):
        t_lo, t_hi = np.nextafter(t_lo, f32(-np.inf)), np.nextafter(t_hi, f32(np.inf))
        amb = amb or theta_decisions(t_lo, dtheta) != own or theta_decisions(t_hi, dtheta) != own
    return theta, int(amb)


def search_pair(kf, grid, fr, i, level, desc, th, counters=None, double_overload=False):
    """:2122-2263 for line i of `fr` = front(...) -> (reached, bestIdx, bestDist, candidates whose distance was taken, theta's mark)."""
    nx, ny, d, n2 = representation(fr["uS"][i], fr["vS"][i], fr["uE"][i], fr["vE"][i])
    if n2 == 0:
        if counters is not None:
            counters["end_points_coincide"] += 1
        return DEGENERATE, -1, 256, 0, 0
    theta = atan2_host(ny, nx, double_overload)
    scale = np.asarray(kf["scale_factors"], f32)[level]
    dtheta = f32(K_DELTA_THETA * scale)
    dd = f32(f32(f32(th) * K_DELTA_D) * scale)
    amb = theta_rule(ny, nx, dtheta)[1]
    ind, wrapped = window(kf, grid, theta, d, dtheta, dd, counters)
    if ind is None:
        return FULL_THETA, -1, 256, 0, amb
    if len(ind) == 0:
        return EMPTY_WINDOW, -1, 256, 0, amb
    kl = kf["kl"][ind]
    oct_ = kl["octave"].astype(np.int64)
    below, above = oct_ < level - 1, oct_ > level
    band = ~(below | above)
    sig = np.asarray(kf["inv_level_sigma2"], f32)[np.clip(oct_, 0, len(kf["inv_level_sigma2"]) - 1)]
    sx, sy, ex, ey = kl["startPointX"], kl["startPointY"], kl["endPointX"], kl["endPointY"]
    with np.errstate(all="ignore"):
        ds = (nx * sx + ny * sy) - d
        de = (nx * ex + ny * ey) - d
        drop_s, drop_e = (ds * ds) * sig > CHI2, (de * de) * sig > CHI2
        if kf["u_right_start"] is None:
            stereo = np.zeros(len(ind), bool)
            drop_r = stereo
            urs = ure = None
        else:
            urs, ure = np.asarray(kf["u_right_start"], f32)[ind], np.asarray(kf["u_right_end"], f32)[ind]
            stereo = (urs >= 0) & (ure >= 0)
            mbf = f32(kf["mbf"])
            rnx, rny, rd, _ = representation(fr["uS"][i] - mbf * fr["invSz"][i], fr["vS"][i], fr["uE"][i] - mbf * fr["invEz"][i], fr["vE"][i])
            dsr = (rnx * urs + rny * sy) - rd
            der = (rnx * ure + rny * ey) - rd
            drop_r = stereo & (((dsr * dsr) * sig > CHI2) | ((der * der) * sig > CHI2))
    ok = band & ~drop_s & ~drop_e & ~drop_r
    if counters is not None:
        counters["dropped_below_level"] += int(below.sum())
        counters["dropped_above_level"] += int(above.sum())
        counters["dropped_start_gate_alone"] += int((band & drop_s & ~drop_e).sum())
        counters["dropped_end_gate_alone"] += int((band & ~drop_s & drop_e).sum())
        counters["dropped_right_gate_alone"] += int((band & ~drop_s & ~drop_e & drop_r).sum())
        if urs is None:
            counters["u_right_empty"] += 1
        else:
            counters["u_right_start_zero_stereo_branch"] += int((band & ~drop_s & ~drop_e & stereo & (urs == 0)).sum())
            counters["u_right_end_negative_skips_stereo"] += int((band & ~drop_s & ~drop_e & (urs >= 0) & (ure < 0)).sum())
    cand = ind[ok]
    if len(cand) == 0:
        return NO_CANDIDATE, -1, 256, 0, amb
    dist = _POP[np.bitwise_xor(np.asarray(kf["desc"], np.uint8)[cand], np.asarray(desc, np.uint8)[None, :])].sum(1)
    j = int(np.argmin(dist))            # the first minimum
    best, best_idx = int(dist[j]), int(cand[j])
    if counters is not None:
        tied = dist == best
        if best <= TH_LOW and tied.sum() > 1 and wrapped[ok][j] and best_idx == cand[tied].max() and best_idx != cand[tied].min():
            counters["tie_winner_in_wrapped_part_higher_index"] += 1
        counters["best_dist_60"] += best == 60
        counters["best_dist_61"] += best == 61
        counters["beyond_member_64"] += int(np.flatnonzero(ind == best_idx)[0]) >= 64
    return (CANDIDATE if best <= TH_LOW else ABOVE_TH_LOW), best_idx, best, len(cand), amb


def fuse_search(kfs, lines, skip, th, counters=None, log_double=False, atan_double=False):
    """-> dict of [K, M] arrays: best_idx / best_dist (the entries' outputs), reached, raw_best_idx / raw_best_dist (bestIdx, bestDist
    as the loop left them: -1 / 256 without a candidate), n_dist (descriptor distances taken), level (-1 before PredictScale), ambiguous
    (the level's or theta's mark), n_proj (projectLinear calls: 0 .. 3), proj (uM, vM, uS, vS, uE, vE as far as the projection got, 0 beyond)."""
    K, M = len(kfs), len(np.asarray(lines["max_dist"]))
    o = dict(best_idx=np.full((K, M), -1, np.int32), best_dist=np.full((K, M), -1, np.int32), reached=np.zeros((K, M), np.uint8),
             raw_best_idx=np.full((K, M), -1, np.int32), raw_best_dist=np.full((K, M), 256, np.int32), n_dist=np.zeros((K, M), np.int32),
             level=np.full((K, M), -1, np.int32), ambiguous=np.zeros((K, M), np.uint8), proj=np.zeros((K, M, 6), f32),
             n_proj=np.zeros((K, M), np.int32))
    if counters is not None:
        for k in REACHED + SUB_FACTS + ("ambiguous_level", "ambiguous_theta"):
            counters.setdefault(k, 0)
    desc = np.asarray(lines["desc"], np.uint8).reshape(-1, 32)
    for k, kf in enumerate(kfs):
        grid = grid_of(kf, atan_double)
        fr = front(kf, lines)
        lsf, levels = f32(kf["log_scale_factor"]), len(kf["scale_factors"])
        for i in range(M):
            if skip is not None and skip[k][i]:
                reached = SKIPPED
            else:
                reached = int(fr["reached"][i])
                n_proj = 0 if reached == MIDDLE_BEHIND else (1 if reached < END_OUTSIDE else (
                    2 if reached == END_OUTSIDE and _outside(kf, fr["uS"][i], fr["vS"][i]) else 3))
                o["n_proj"][k, i] = n_proj
                o["proj"][k, i, :2 * n_proj] = [fr[c][i] for c in ("uM", "vM", "uS", "vS", "uE", "vE")][:2 * n_proj]
                if counters is not None and reached == DEGENERATE:
                    counters["dist_zero"] += 1
                if reached == EMPTY_WINDOW:
                    level = predict_scale(fr["ratio"][i], lsf, levels, log_double)[0]
                    o["level"][k, i] = level
                    amb_level = rule(fr["ratio"][i], lsf, levels)[1]
                    reached, bi, bd, nd, amb_theta = search_pair(kf, grid, fr, i, level, desc[i], th, counters, atan_double)
                    o["ambiguous"][k, i] = int(bool(amb_level or amb_theta))
                    o["raw_best_idx"][k, i], o["raw_best_dist"][k, i], o["n_dist"][k, i] = bi, bd, nd
                    if reached == CANDIDATE:
                        o["best_idx"][k, i], o["best_dist"][k, i] = bi, bd
                    if counters is not None:
                        counters["ambiguous_level"] += int(amb_level)
                        counters["ambiguous_theta"] += int(amb_theta)
            o["reached"][k, i] = reached
            if counters is not None and reached < len(REACHED):
                counters[REACHED[reached]] += 1
    return o


def _outside(kf, u, v):
    b = np.asarray(kf["bounds4"], f32)
    return bool(u < b[0] or u > b[1] or v < b[2] or v > b[3])
