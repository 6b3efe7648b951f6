"""Flat restatement of Frame::ComputeStereoFromRGBD (reference src/Frame.cc:2251-2279), Frame::ComputeStereoLinesFromRGBD
(:2434-2674, the live CHECK_RGBD_ENDPOINTS_DEPTH_CONSISTENCY path, with computeLocalMinDepth / computeLocalMinMaxDepth
:2311-2370) and Frame::ComputeSceneMedianDepth (:2730-2751) in numpy scalars: np.float32 where the reference computes in
float, np.float64 where it builds Eigen::Vector3d, every operation in the reference's order (sums of three as
c0 + (c1 + c2), Eigen's unrolled reduction), with a counter per branch.  tests/golden/frame_rgbd_reference.npz — the
reference's own run (scripts/make_frame_rgbd_golden.py) — pins it bit for bit; the device code is held to the same file."""
import math

import numpy as np

F32, F64 = np.float32, np.float64
FLT_MAX = np.finfo(np.float32).max
MAX_MISALIGNMENT = F32(0.03)                                  # Frame::kLinePointsMaxMisalignment
COS_VIEW_Z_ANGLE_MAX = F32(math.cos(30. * math.pi / 180.))    # Frame::kCosViewZAngleMax
BRANCHES = ("no_end_point", "no_middle", "misaligned", "repaired_emax", "repaired_smax", "rejected", "short", "view_angle", "stereo")


def _trunc(f):
    return int(f)        # float -> int as the reference's `const int&` parameters bind it


def local_min_max(depth, u, v):
    """computeLocalMinMaxDepth with delta 1 -> (min, max) of the finite values > 0 in the clipped 3 x 3 window, 0 if none."""
    h, w = depth.shape
    mn, mx = FLT_MAX, F32(0)
    for du in (-1, 0, 1):
        for dv in (-1, 0, 1):
            ou, ov = u + du, v + dv
            if 0 <= ou < w and 0 <= ov < h:
                val = depth[ov, ou]
                if np.isfinite(val) and val > 0:
                    if mn > val:
                        mn = val
                    if mx < val:
                        mx = val
    return (mn if mn < FLT_MAX else F32(0)), (mx if mx > 0 else F32(0))


def _v3(a, b, c):
    return (F64(a), F64(b), F64(c))


def _cross(a, b):
    return (a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0])


def _sqnorm(a):
    return a[0] * a[0] + (a[1] * a[1] + a[2] * a[2])


def _norm(a):
    return np.sqrt(_sqnorm(a))


def _dot(a, b):
    return a[0] * b[0] + (a[1] * b[1] + a[2] * b[2])


def _normalized(a):
    z2 = _sqnorm(a)
    if not z2 > 0:
        return a
    s = np.sqrt(z2)
    return (a[0] / s, a[1] / s, a[2] / s)


def stereo_from_rgbd(kps_xy, kps_un_x, depth, mbf):
    """-> (mvuRight, mvDepth).  depth: the image (height x width view, any pitch)."""
    n = len(kps_xy)
    ur, z = np.full(n, -1, F32), np.full(n, -1, F32)
    mbf = F32(mbf)
    h, w = depth.shape
    with np.errstate(all="ignore"):
        for i in range(n):
            u, v = _trunc(kps_xy[i][0]), _trunc(kps_xy[i][1])
            if not (0 <= u < w and 0 <= v < h):
                continue                 # (undefined in the reference; the library writes -1)
            d = depth[v, u]
            if d > 0:
                z[i] = d
                ur[i] = F32(kps_un_x[i]) - mbf / d
    return ur, z


def scene_median_depth(depths, fallback=1.5):
    v = np.sort(np.asarray(depths, F32)[np.asarray(depths, F32) > 0])
    return F32(v[(len(v) - 1) // 2]) if len(v) else F32(fallback)


def stereo_lines_from_rgbd(lines8, depth, K4, mbf, min_line_length_3d=0.01, counters=None):
    """lines8[i] = uS vS uE vE of mvKeyLines[i], then of mvKeyLinesUn[i] -> (uRightStart, depthStart, uRightEnd, depthEnd)."""
    n = len(lines8)
    out = [np.full(n, -1, F32) for _ in range(4)]
    cnt = counters if counters is not None else {}
    for k in BRANCHES:
        cnt.setdefault(k, 0)
    fx, fy, cx, cy = (F32(x) for x in K4)
    invfx, invfy = F32(1) / fx, F32(1) / fy
    mbf, min_len, half = F32(mbf), F64(F32(min_line_length_3d)), F32(0.5)
    with np.errstate(all="ignore"):
        for i in range(n):
            uS, vS, uE, vE, uSU, vSU, uEU, vEU = (F32(x) for x in lines8[i])
            vM, uM = half * (vS + vE), half * (uS + uE)
            vMU, uMU = half * (vSU + vEU), half * (uSU + uEU)
            dS, dSmax = local_min_max(depth, _trunc(uS), _trunc(vS))
            dE, dEmax = local_min_max(depth, _trunc(uE), _trunc(vE))
            dM, _ = local_min_max(depth, _trunc(uM), _trunc(vM))
            if dS > 0 and dE > 0:
                xS, yS = (uSU - cx) * dS * invfx, (vSU - cy) * dS * invfy
                xE, yE = (uEU - cx) * dE * invfx, (vEU - cy) * dE * invfy
                lineES = _v3(xS - xE, yS - yE, dS - dE)
                if dM > 0:
                    xM, yM = (uMU - cx) * dM * invfx, (vMU - cy) * dM * invfy
                    lineMS = _v3(xS - xM, yS - yM, dS - dM)
                    lineEM = _v3(xM - xE, yM - yE, dM - dE)
                    dist = F32(_norm(_cross(lineMS, lineEM)) / _norm(lineES))
                    if dist > MAX_MISALIGNMENT:
                        cnt["misaligned"] += 1
                        if dEmax > 0:
                            scale = dEmax / dE
                            xEmax, yEmax = xE * scale, yE * scale
                            lineEmaxM = _v3(xM - xEmax, yM - yEmax, dM - dEmax)
                            lineEmaxS = _v3(xS - xEmax, yS - yEmax, dS - dEmax)
                            d2 = F32(_norm(_cross(lineMS, lineEmaxM)) / _norm(lineEmaxS))
                            if d2 < MAX_MISALIGNMENT and d2 < dist:
                                cnt["repaired_emax"] += 1
                                xE, yE, dE = xEmax, yEmax, dEmax
                                lineEM, lineES, dist = lineEmaxM, lineEmaxS, d2
                        if dSmax > 0:
                            scale = dSmax / dS
                            xSmax, ySmax = xS * scale, yS * scale
                            lineMSmax = _v3(xSmax - xM, ySmax - yM, dSmax - dM)
                            lineESmax = _v3(xSmax - xE, ySmax - yE, dSmax - dE)
                            d2 = F32(_norm(_cross(lineMSmax, lineEM)) / _norm(lineESmax))
                            if d2 < MAX_MISALIGNMENT and d2 < dist:
                                cnt["repaired_smax"] += 1
                                xS, yS, dS = xSmax, ySmax, dSmax
                                lineMS, lineES, dist = lineMSmax, lineESmax, d2
                    if dist > MAX_MISALIGNMENT:
                        cnt["rejected"] += 1
                        dS = dE = F32(-1)
                else:
                    cnt["no_middle"] += 1
                if _norm(lineES) < min_len:
                    cnt["short"] += 1
                    dS = dE = F32(-1)
                if dS > 0 and dE > 0:
                    ray = _normalized(_v3(xS, yS, dS))
                    direction = _normalized(_v3(xS - xE, yS - yE, dS - dE))
                    if np.abs(F32(_dot(ray, direction))) > COS_VIEW_Z_ANGLE_MAX:
                        cnt["view_angle"] += 1
                        dS = dE = F32(-1)
            else:
                cnt["no_end_point"] += 1
            if dS > 0 and np.isfinite(dS) and dE > 0 and np.isfinite(dE):
                cnt["stereo"] += 1
                out[0][i], out[1][i] = uSU - mbf / dS, dS
                out[2][i], out[3][i] = uEU - mbf / dE, dE
    return tuple(out)
