"""numpy restatement of Frame::isInFrustum(MapPointPtr&, viewingCosLimit) / (MapLinePtr&, viewingCosLimit) (reference
src/Frame.cc:955-1017, :1033-1142) with MapPoint / MapLine::PredictScale, in the reference's f32 sequence and the evaluation
order of Eigen 3.3 for fixed sizes (sums of three as c0 + (c1 + c2)), with one counter per branch.  Pinned bit for bit by
tests/golden/track_local_reference.npz (tests/test_track_local.py) before its counters are believed; it then recomputes the
golden at other sizes.  The logarithm of PredictScale is the C library's logf, called per element: numpy's own float32 log is
another implementation."""
import ctypes
import ctypes.util
import math

import numpy as np

f32 = np.float32
_libm = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
_libm.logf.restype = ctypes.c_float
_libm.logf.argtypes = [ctypes.c_float]
_libm.log.restype = ctypes.c_double
_libm.log.argtypes = [ctypes.c_double]

POINT_BRANCHES = ("skipped", "behind", "pcz_zero", "out_left", "out_right", "out_top", "out_bottom", "too_near", "too_far", "grazing",
                  "in_view", "level_below_0", "level_at_0", "level_above_top", "view_cos_above_998", "view_cos_below_998", "ambiguous")
LINE_BRANCHES = ("skipped", "behind", "out_left", "out_right", "out_top", "out_bottom", "too_near", "near_quirk", "too_far", "grazing",
                 "in_view", "level_below_0", "level_above_top", "end_behind", "ambiguous")


def predict_scale(ratio, lsf, levels, double_overload=False):
    """-> (level, unclamped nScale).  ratio, lsf: np.float32."""
    if double_overload:
        q = _libm.log(float(ratio)) / float(lsf)
    else:
        q = f32(f32(_libm.logf(float(ratio))) / f32(lsf))
    n = int(math.ceil(q)) if math.isfinite(q) else -2 ** 31
    return (0 if n < 0 else (levels - 1 if n >= levels else n)), n


def rule(ratio, lsf, levels):
    """plvs::predict_level (plvs_amd/csrc/track_level.hpp) -> (level, ambiguous)."""
    with np.errstate(all="ignore"):
        q = math.log(float(ratio)) / float(lsf) if ratio > 0 else float("nan")
    if not q > -1.0:
        return 0, 0
    if q > levels:
        return levels - 1, 0
    up, nearest = math.ceil(q), math.floor(q + 0.5)
    eps = 6.0 * 2.0 ** -23 * abs(q) + 2.0 ** -40
    lv = 0 if up < 0 else (levels - 1 if up >= levels else int(up))
    return lv, int(abs(q - nearest) <= eps and 0 <= nearest <= levels - 2)


def _cam(Rcw, tcw, p):
    """mRcw * P + mtcw; Rcw: 9 floats, column-major.  p: [m, 3] f32."""
    R = np.asarray(Rcw, f32)
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    return np.stack([(R[0] * x + (R[3] * y + R[6] * z)) + f32(tcw[0]), (R[1] * x + (R[4] * y + R[7] * z)) + f32(tcw[1]),
                     (R[2] * x + (R[5] * y + R[8] * z)) + f32(tcw[2])], 1).astype(f32)


def _norm(v):
    return np.sqrt(v[:, 0] * v[:, 0] + (v[:, 1] * v[:, 1] + v[:, 2] * v[:, 2])).astype(f32)


def _project(K4, c):
    K4 = np.asarray(K4, f32)
    return (K4[0] * c[:, 0] / c[:, 2] + K4[2]).astype(f32), (K4[1] * c[:, 1] / c[:, 2] + K4[3]).astype(f32)


def _tests(cam, world, camp, normal, min_d, max_d, skip, C, line_min=None):
    """The shared tests -> (ok, passed_bounds, u, v, dist, view_cos)."""
    b = np.asarray(cam["bounds4"], f32)
    u, v = _project(cam["K4"], camp)
    PO = (world - np.asarray(cam["Ow"], f32)[None, :]).astype(f32)
    dist = _norm(PO)
    vcos = ((PO[:, 0] * normal[:, 0] + (PO[:, 1] * normal[:, 1] + PO[:, 2] * normal[:, 2])) / dist).astype(f32)
    m = len(world)
    ok, stage = np.zeros(m, bool), np.zeros(m, bool)
    for k in range(m):
        if skip[k]:
            C["skipped"] += 1
            continue
        if camp[k, 2] < 0:
            C["behind"] += 1
            continue
        if "pcz_zero" in C and camp[k, 2] == 0:
            C["pcz_zero"] += 1
        if u[k] < b[0]:
            C["out_left"] += 1
            continue
        if u[k] > b[1]:
            C["out_right"] += 1
            continue
        if v[k] < b[2]:
            C["out_top"] += 1
            continue
        if v[k] > b[3]:
            C["out_bottom"] += 1
            continue
        stage[k] = True
        if dist[k] < min_d[k]:
            C["too_near"] += 1
            if line_min is not None and dist[k] >= f32(0.8) * line_min[k]:
                C["near_quirk"] += 1
            continue
        if dist[k] > max_d[k]:
            C["too_far"] += 1
            continue
        if dist[k] == 0:
            continue
        if vcos[k] < f32(cam["viewing_cos_limit"]):
            C["grazing"] += 1
            continue
        ok[k] = True
        C["in_view"] += 1
    return ok, stage, u, v, dist, vcos


def is_in_frustum(cam, points=None, lines=None, counters=None):
    """cam: dict(K4, mbf, bounds4, Rcw, tcw, Ow, viewing_cos_limit, log_scale_factor, n_levels, line_log_scale_factor,
    n_line_levels); points: dict(skip, pos, normal, min_dist, max_dist); lines: dict(skip, start, end, normal, max_dist[, min_dist]).
    -> dict of the output arrays of plvs_hip_frame_is_in_frustum (prefix p_ / l_), n_in_view_points, n_in_view_lines."""
    out = {}
    mbf = f32(cam["mbf"])
    CP, CL = {k: 0 for k in POINT_BRANCHES}, {k: 0 for k in LINE_BRANCHES}
    with np.errstate(all="ignore"):
        if points is not None:
            pos, normal = np.asarray(points["pos"], f32).reshape(-1, 3), np.asarray(points["normal"], f32).reshape(-1, 3)
            m = len(pos)
            Pc = _cam(cam["Rcw"], cam["tcw"], pos)
            Pc_dist = _norm(Pc)
            invz = (f32(1.0) / Pc[:, 2]).astype(f32)
            mn, mx = (f32(0.8) * np.asarray(points["min_dist"], f32)).astype(f32), (f32(1.2) * np.asarray(points["max_dist"], f32)).astype(f32)
            ok, stage, u, v, dist, vcos = _tests(cam, pos, Pc, normal, mn, mx, points["skip"], CP)
            o = dict(in_view=ok.astype(np.uint8), proj_x=np.where(stage, u, f32(-1)).astype(f32), proj_y=np.where(stage, v, f32(-1)).astype(f32),
                     proj_xr=np.where(ok, u - mbf * invz, f32(0)).astype(f32), track_depth=np.where(ok, Pc_dist, f32(0)).astype(f32),
                     level=np.zeros(m, np.int32), view_cos=np.where(ok, vcos, f32(0)).astype(f32), ambiguous=np.zeros(m, np.uint8),
                     ratio=np.zeros(m, f32))
            for k in np.flatnonzero(ok):
                ratio = f32(f32(points["max_dist"][k]) / dist[k])
                o["level"][k], n = predict_scale(ratio, f32(cam["log_scale_factor"]), cam["n_levels"])
                o["ratio"][k] = ratio
                o["ambiguous"][k] = rule(ratio, f32(cam["log_scale_factor"]), cam["n_levels"])[1]
                CP["ambiguous"] += int(o["ambiguous"][k])
                CP["level_below_0"] += n < 0
                CP["level_at_0"] += n == 0
                CP["level_above_top"] += n >= cam["n_levels"]
                CP["view_cos_above_998"] += float(vcos[k]) > 0.998
                CP["view_cos_below_998"] += not float(vcos[k]) > 0.998
            out.update({"p_" + k: a for k, a in o.items()})
            out["n_in_view_points"] = int(ok.sum())
        if lines is not None:
            S, E = np.asarray(lines["start"], f32).reshape(-1, 3), np.asarray(lines["end"], f32).reshape(-1, 3)
            normal = np.asarray(lines["normal"], f32).reshape(-1, 3)
            m = len(S)
            mid = (f32(0.5) * (S + E)).astype(f32)
            Mc = _cam(cam["Rcw"], cam["tcw"], mid)
            mxd = np.asarray(lines["max_dist"], f32)
            line_min = np.asarray(lines.get("min_dist", np.zeros(m)), f32)
            ok, _, _, _, dist, vcos = _tests(cam, mid, Mc, normal, (f32(0.8) * mxd).astype(f32), (f32(1.2) * mxd).astype(f32), lines["skip"], CL,
                                             line_min=line_min)
            Sc, Ec = _cam(cam["Rcw"], cam["tcw"], S), _cam(cam["Rcw"], cam["tcw"], E)
            us, vs = _project(cam["K4"], Sc)
            ue, ve = _project(cam["K4"], Ec)
            proj = np.zeros((m, 6), f32)
            proj[:, :4] = -1
            proj_xr = np.full((m, 2), -1, f32)
            full = np.stack([us, vs, ue, ve, Sc[:, 2], Ec[:, 2]], 1).astype(f32)
            xr = np.stack([us - mbf * (f32(1.0) / Sc[:, 2]), ue - mbf * (f32(1.0) / Ec[:, 2])], 1).astype(f32)
            proj[ok], proj_xr[ok] = full[ok], xr[ok]
            o = dict(in_view=ok.astype(np.uint8), proj=proj, proj_xr=proj_xr, level=np.zeros(m, np.int32),
                     view_cos=np.where(ok, vcos, f32(0)).astype(f32), ambiguous=np.zeros(m, np.uint8), ratio=np.zeros(m, f32))
            for k in np.flatnonzero(ok):
                ratio = f32(mxd[k] / dist[k])
                o["level"][k], n = predict_scale(ratio, f32(cam["line_log_scale_factor"]), cam["n_line_levels"])
                o["ratio"][k] = ratio
                o["ambiguous"][k] = rule(ratio, f32(cam["line_log_scale_factor"]), cam["n_line_levels"])[1]
                CL["ambiguous"] += int(o["ambiguous"][k])
                CL["level_below_0"] += n < 0
                CL["level_above_top"] += n >= cam["n_line_levels"]
                CL["end_behind"] += bool(Sc[k, 2] < 0 or Ec[k, 2] < 0)
            out.update({"l_" + k: a for k, a in o.items()})
            out["n_in_view_lines"] = int(ok.sum())
    if counters is not None:
        counters["points"] = {k: int(v) for k, v in CP.items()}
        counters["lines"] = {k: int(v) for k, v in CL.items()}
    return out
