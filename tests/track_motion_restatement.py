"""numpy restatement of the projection stage of plvs_hip_frame_search_last_frame and of the retry rules around the two searches,
held bit for bit against the reference's compiled definitions by tests/test_track_motion.py (tests/golden/track_motion_reference.npz,
scripts/make_track_motion_golden.py) before any test relies on it at other sizes.

Points (src/ORBmatcher.cc:1805-1820): Tcw * x3Dw is Sophus' quaternion action (Thirdparty/Sophus/sophus/so3.hpp:363-366,
se3.hpp:323) — uv = q.vec x p; uv += uv; pc = (p + w uv) + q.vec x uv; pc += t —, invzc = 1.0 / x3Dc(2) in f64 rounded to f32,
Pinhole::project = fx * x / z + cx, the four comparisons (a NaN passes).  Lines: LineProjection::ProjectLineWithCheck
(include/LineProjection.h:144-264) for a pinhole camera.  Every operation is one f32 numpy operation: no contraction."""
import numpy as np

f32 = np.float32


def _cross(a, b):
    return np.stack([a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1], a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2], a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]], -1)


def se3_act(q, t, p):
    """Sophus::SE3f(q, t) * p for p [n, 3] (f32)."""
    q, t, p = np.asarray(q, f32), np.asarray(t, f32), np.asarray(p, f32).reshape(-1, 3)
    v = np.broadcast_to(q[:3], p.shape)
    uv = _cross(v, p)
    uv = uv + uv
    c = _cross(v, uv)
    return ((p + q[3] * uv) + c) + t[None, :]


def matrix_act(Rcw, t, p):
    """mRcw * p + mtcw as Eigen 3.3 evaluates it for fixed sizes (Rcw: 9 floats, column-major): NOT what the point search runs."""
    R, t, p = np.asarray(Rcw, f32), np.asarray(t, f32), np.asarray(p, f32).reshape(-1, 3)
    return np.stack([(R[r] * p[:, 0] + (R[3 + r] * p[:, 1] + R[6 + r] * p[:, 2])) + t[r] for r in range(3)], -1)


def _project(K4, pc):
    K4 = np.asarray(K4, f32)
    return K4[0] * pc[:, 0] / pc[:, 2] + K4[2], K4[1] * pc[:, 1] / pc[:, 2] + K4[3]


def _outside(b, u, v):
    return (u < b[0]) | (u > b[1]) | (v < b[2]) | (v > b[3])


def direction(poses):
    """bForward, bBackward (src/ORBmatcher.cc:1788-1795)."""
    tlc = se3_act(poses["q_lw"], poses["tlw"], np.asarray(poses["Ow"], f32))[0]
    mono = bool(poses.get("mono", 0))
    return int(tlc[2] > f32(poses["mb"]) and not mono), int(-tlc[2] > f32(poses["mb"]) and not mono)


def project_points(poses, points, counters=None, act=None):
    """-> dict(pc [n, 3] (x3Dc; 0 where not valid), proj_valid, u, v, invz) in the layout of plvs_motion_points' outputs."""
    valid = np.asarray(points["valid"], np.uint8) != 0
    n = len(valid)
    b = np.asarray(poses["bounds4"], f32)
    with np.errstate(all="ignore"):
        pc = (se3_act(poses["q_cw"], poses["tcw"], points["pos"]) if act is None else act(points["pos"])).astype(f32)
        invz = (1.0 / pc[:, 2].astype(np.float64)).astype(f32)
        front = valid & ~(invz < 0)
        u, v = _project(poses["K4"], pc)
        out = _outside(b, u, v)
    ok = front & ~out
    res = dict(pc=np.where(valid[:, None], pc, f32(0)).astype(f32), proj_valid=ok.astype(np.uint8), u=np.where(front, u, f32(-1)).astype(f32), v=np.where(front, v, f32(-1)).astype(f32),
               invz=np.where(valid, invz, f32(0)).astype(f32))
    if counters is not None:
        with np.errstate(all="ignore"):
            counters.update(invalid=int((~valid).sum()), behind=int((valid & (pc[:, 2] < 0)).sum()),
                            z_minus_zero=int((valid & (pc[:, 2] == 0) & np.signbit(pc[:, 2])).sum()),
                            z_plus_zero_nan=int((front & (pc[:, 2] == 0) & (np.isnan(u) | np.isnan(v))).sum()),
                            z_plus_zero_inf=int((front & (pc[:, 2] == 0) & ~(np.isnan(u) | np.isnan(v))).sum()),
                            nan_accepted=int((ok & (np.isnan(u) | np.isnan(v))).sum()),
                            out_left=int((front & (u < b[0])).sum()), out_right=int((front & (u > b[1])).sum()),
                            out_top=int((front & ~(u < b[0]) & ~(u > b[1]) & (v < b[2])).sum()),
                            out_bottom=int((front & ~(u < b[0]) & ~(u > b[1]) & (v > b[3])).sum()),
                            on_left=int((ok & (u == b[0])).sum()), on_right=int((ok & (u == b[1])).sum()),
                            on_top=int((ok & (v == b[2])).sum()), on_bottom=int((ok & (v == b[3])).sum()), accepted=int(ok.sum()))
    return res


def project_lines(poses, lines, counters=None):
    """-> dict(proj_valid, proj6 [n, 6]) in the layout of plvs_motion_lines' outputs: the stores of ProjectLineWithCheck in its
    order, from (-1, -1, -1, -1, 0, 0)."""
    valid = np.asarray(lines["valid"], np.uint8) != 0
    n = len(valid)
    b = np.asarray(poses["bounds4"], f32)
    KL = poses.get("K4_linear")
    KL = np.asarray(poses["K4"] if KL is None else KL, f32)
    S, E = np.asarray(lines["start"], f32).reshape(n, 3), np.asarray(lines["end"], f32).reshape(n, 3)
    mx = np.asarray(lines["max_dist"], f32)
    with np.errstate(all="ignore"):
        mid = ((S + E) * f32(0.5)).astype(f32)
        Mc, Sc, Ec = (matrix_act(poses["Rcw"], poses["tcw"], x) for x in (mid, S, E))
        a1 = valid & ~(Mc[:, 2] < 0)
        uM, vM = _project(KL, Mc)
        a2 = a1 & ~_outside(b, uM, vM)
        dist = np.sqrt(Mc[:, 0] * Mc[:, 0] + (Mc[:, 1] * Mc[:, 1] + Mc[:, 2] * Mc[:, 2]))
        near, far = dist < f32(0.8) * mx, dist > f32(1.2) * mx
        a3 = a2 & ~near & ~far
        a4 = a3 & ~(Sc[:, 2] < 0)
        a5 = a4 & ~(Ec[:, 2] < 0)          # the stores of the start point happen from here on
        invS, invE = f32(1.0) / Sc[:, 2], f32(1.0) / Ec[:, 2]
        uS, vS = _project(KL, Sc)
        uE, vE = _project(KL, Ec)
        a6 = a5 & ~_outside(b, uS, vS)     # the stores of the end point happen from here on
        a7 = a6 & ~_outside(b, uE, vE)
    proj6 = np.zeros((n, 6), f32)
    proj6[:, :4] = -1
    proj6[a5, 0], proj6[a5, 1], proj6[a5, 4] = uS[a5], vS[a5], invS[a5]
    proj6[a6, 2], proj6[a6, 3], proj6[a6, 5] = uE[a6], vE[a6], invE[a6]
    if counters is not None:
        with np.errstate(all="ignore"):
            counters.update(invalid=int((~valid).sum()), middle_behind=int((valid & ~a1).sum()),
                            middle_out_left=int((a1 & (uM < b[0])).sum()), middle_out_right=int((a1 & (uM > b[1])).sum()),
                            middle_out_top=int((a1 & ~(uM < b[0]) & ~(uM > b[1]) & (vM < b[2])).sum()),
                            middle_out_bottom=int((a1 & ~(uM < b[0]) & ~(uM > b[1]) & (vM > b[3])).sum()),
                            too_near=int((a2 & near).sum()), too_far=int((a2 & ~near & far).sum()),
                            on_near_edge=int((a3 & (dist == f32(0.8) * mx)).sum()), on_far_edge=int((a3 & (dist == f32(1.2) * mx)).sum()),
                            start_behind=int((a3 & ~a4).sum()), end_behind=int((a4 & ~a5).sum()), start_out=int((a5 & ~a6).sum()),
                            end_out=int((a6 & ~a7).sum()), accepted=int(a7.sum()))
    return dict(proj_valid=a7.astype(np.uint8), proj6=proj6, dist=dist.astype(f32))


def track_with_motion_model(search_points, search_lines, th, min_point_matches, min_line_matches, have_lines=True):
    """The retry rules of Tracking::TrackWithMotionModel (src/Tracking.cc:3626-3663) around search_points(th) -> (n, assigned) and
    search_lines(larger) -> (n, assigned).  -> dict(nmatches_points, assigned_points, nmatches_lines, assigned_lines, th_used,
    larger_line_search_used, point_retries, line_retries)."""
    th_used, point_retries, line_retries = th, 0, 0
    n_p, a_p = search_points(th)                                    # :3626
    larger = False                                                  # :3628
    if n_p < min_point_matches:                                     # :3631
        larger = True                                               # :3633
        th_used, point_retries = 2 * th, 1
        n_p, a_p = search_points(2 * th)                            # :3638
    n_l, a_l = 0, None
    if have_lines:                                                  # :3644
        n_l, a_l = search_lines(larger)                             # :3653
        if n_l < min_line_matches and not larger:                   # :3654
            larger, line_retries = True, 1
            n_l, a_l = search_lines(True)                           # :3659
    return dict(nmatches_points=n_p, assigned_points=a_p, nmatches_lines=n_l, assigned_lines=a_l, th_used=th_used,
                larger_line_search_used=int(larger), point_retries=point_retries, line_retries=line_retries)
