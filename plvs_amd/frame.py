"""Points + lines of one frame, extracted concurrently (Frame::Frame's threadLeft /
threadLines, reference src/Frame.cc:503-508).  All compute runs in libplvs_hip.so."""
import ctypes

import torch

from . import _lib
from .lines import LineExtractor
from .orb import ORBextractor

_vp, _i = ctypes.c_void_p, ctypes.c_int
L = _lib.lib
L.plvs_hip_frame_extract_dev.argtypes = [_vp, _vp, _vp, _i, _i, _i, _i, _i, _vp, _vp, _i, _vp, _vp,
                                         _vp, _vp, _i, _vp]


_HOOK = ctypes.CFUNCTYPE(None, _vp, _i)
L.plvs_hip_frame_extract_dev_hook.argtypes = L.plvs_hip_frame_extract_dev.argtypes + [_HOOK, _vp]


def extract_frame(orb: ORBextractor, lines: LineExtractor, image: torch.Tensor, vLappingArea=(0, 0), after_points=None):
    """image: 2-D uint8 CUDA tensor.  -> (monoIndex, keypoints, descriptors, keylines, line descriptors)
    — and, with after_points, a sixth element: what the hook returned (None when it did not run).

    after_points(keypoints, descriptors): called on this thread as soon as the points are out, while the line thread
    is still extracting (what the caller does with the points alone: the ORB SearchByProjection of the tracking
    step)."""
    assert image.is_cuda and image.dtype == torch.uint8 and image.dim() == 2
    torch.cuda.current_stream().synchronize()
    h, w = image.shape
    nk, mono, nl = _i(), _i(), _i()
    args = (orb._h, lines._h, _vp(image.data_ptr()), w, h, image.stride(0), vLappingArea[0], vLappingArea[1],
            _lib.np_ptr(orb._kps), _lib.np_ptr(orb._desc), orb._cap, ctypes.byref(nk), ctypes.byref(mono),
            _lib.np_ptr(lines._kl), _lib.np_ptr(lines._desc), lines._cap, ctypes.byref(nl))
    if after_points is None:
        _lib.check(L.plvs_hip_frame_extract_dev(*args))
    else:
        failure, hooked = [], [None]

        def hook(_user, status):
            if status != 0 or nk.value > orb._cap:
                return
            try:
                hooked[0] = after_points(orb._kps[:nk.value], orb._desc[:nk.value])
            except BaseException as e:      # (an exception must not unwind through the C frame)
                failure.append(e)

        _lib.check(L.plvs_hip_frame_extract_dev_hook(*args, _HOOK(hook), None))
        if failure:
            raise failure[0]
    if nk.value > orb._cap or nl.value > lines._cap:
        raise RuntimeError("extract_frame: output capacity exceeded")
    out = (mono.value, orb._kps[:nk.value].copy(), orb._desc[:nk.value].copy(),
           lines._kl[:nl.value].copy(), lines._desc[:nl.value].copy())
    return out if after_points is None else out + (hooked[0],)


# ---------------------------------------------------------------------------------------------- Frame glue
# What Frame::Frame runs between ExtractORB / ExtractLSD and the first search (src/Frame.cc:541-580).  K = (fx, fy, cx, cy);
# dist = mDistCoef (4, 5 or 8 coefficients; None / first coefficient 0: no distortion).
def _calib(K, dist):
    import numpy as np
    K4 = np.ascontiguousarray(K, np.float32).reshape(4)
    d = None if dist is None else np.ascontiguousarray(dist, np.float32).reshape(-1)
    return K4, d, 0 if d is None else int(d.shape[0])


def UndistortKeyPoints(kps, K, dist):
    """Frame::UndistortKeyPoints (src/Frame.cc:1507-1552): mvKeys -> mvKeysUn (KP_DTYPE records)."""
    import numpy as np
    from .orb import KP_DTYPE
    kps = np.ascontiguousarray(kps, KP_DTYPE)
    un = np.empty_like(kps)
    K4, d, nd = _calib(K, dist)
    f = L.plvs_hip_frame_undistort_keypoints
    f.argtypes = [_vp, _i, _vp, _vp, _i, _vp]
    _lib.check(f(_lib.np_ptr(kps), len(kps), _lib.np_ptr(K4), _lib.np_ptr(d), nd, _lib.np_ptr(un)))
    return un


def ComputeImageBounds(width, height, K, dist):
    """Frame::ComputeImageBounds (src/Frame.cc:1749-1778) -> (mnMinX, mnMaxX, mnMinY, mnMaxY, mnMaxDiag)."""
    import numpy as np
    b = np.zeros(5, np.float32)
    K4, d, nd = _calib(K, dist)
    f = L.plvs_hip_frame_compute_image_bounds
    f.argtypes = [_i, _i, _vp, _vp, _i, _vp]
    _lib.check(f(int(width), int(height), _lib.np_ptr(K4), _lib.np_ptr(d), nd, _lib.np_ptr(b)))
    return tuple(float(x) for x in b)


def UndistortKeyLines(keylines, K, dist, bounds):
    """Frame::UndistortKeyLines (src/Frame.cc:1555-1700, single pinhole camera) -> (mvKeyLinesUn, kept): the undistorted
    lines that stay inside bounds = (mnMinX, mnMaxX, mnMinY, mnMaxY) and the indices of the input lines behind them (the
    caller compacts mvKeyLines / mLineDescriptors with `kept`)."""
    import numpy as np
    kl = np.ascontiguousarray(keylines)
    assert kl.dtype.itemsize == 68
    un = np.empty_like(kl)
    kept = np.zeros(max(len(kl), 1), np.int32)
    n = _i()
    K4, d, nd = _calib(K, dist)
    b = np.ascontiguousarray(bounds, np.float32)[:4].copy()
    f = L.plvs_hip_frame_undistort_keylines
    f.argtypes = [_vp, _i, _vp, _vp, _i, _vp, _vp, _vp, _vp]
    _lib.check(f(_lib.np_ptr(kl), len(kl), _lib.np_ptr(K4), _lib.np_ptr(d), nd, _lib.np_ptr(b), _lib.np_ptr(un), _lib.np_ptr(kept),
                 ctypes.byref(n)))
    return un[:n.value].copy(), kept[:n.value].copy()


def AssignFeaturesToGrid(kps_un, min_x, min_y, grid_w_inv, grid_h_inv):
    """Frame::AssignFeaturesToGrid (src/Frame.cc:716-746), the key-point grid as a CSR -> (cell_start [3073], cell_items):
    cell = column * 48 + row (mGrid[ix][iy]), members in key-point order."""
    import numpy as np
    from .orb import KP_DTYPE
    kps = np.ascontiguousarray(kps_un, KP_DTYPE)
    start = np.zeros(64 * 48 + 1, np.int32)
    items = np.zeros(max(len(kps), 1), np.int32)
    n = _i()
    f = L.plvs_hip_frame_assign_features_to_grid
    f.argtypes = [_vp, _i, ctypes.c_float, ctypes.c_float, ctypes.c_float, ctypes.c_float, _vp, _vp, _vp]
    _lib.check(f(_lib.np_ptr(kps), len(kps), float(min_x), float(min_y), float(grid_w_inv), float(grid_h_inv), _lib.np_ptr(start),
                 _lib.np_ptr(items), ctypes.byref(n)))
    return start, items[:n.value].copy()


# ---------------------------------------------------------------------------------------------- Frame glue, RGB-D
# The two calls that make a frame RGB-D (src/Frame.cc:549, :572) and the RGB-D constructor (:401-600) as one call.  The depth
# image is float32 metres: a numpy array goes through the host flavours (which upload the whole image), a torch CUDA tensor
# — possibly a pitched view, stride(1) == 1 — through the one-launch device flavour, and is the same buffer the TSDF depth
# entries take.
SK_MIN_LINE_LENGTH_3D = 0.01      # Frame::skMinLineLength3D (src/Frame.cc:115)
SK_FOV_CENTER_DISTANCE = 1.5      # KeyFrame::skFovCenterDistance
_f = ctypes.c_float
L.plvs_hip_frame_compute_stereo_from_rgbd.argtypes = [_vp, _vp, _i, _vp, _i, _i, _i, _f, _vp, _vp]
L.plvs_hip_frame_compute_stereo_lines_from_rgbd.argtypes = [_vp, _vp, _i, _vp, _i, _i, _i, _vp, _f, _f, _vp, _vp, _vp, _vp]
L.plvs_hip_frame_stereo_from_rgbd_dev.argtypes = [_vp, _vp, _i, _vp, _vp, _i, _vp, _i, _i, _i, _vp, _f, _f] + [_vp] * 7
L.plvs_hip_frame_scene_median_depth.argtypes = [_vp, _i, _f, _vp]


class RgbdCalib(ctypes.Structure):      # plvs_rgbd_calib
    _fields_ = [("K4", _f * 4), ("dist", _f * 8), ("ndist", ctypes.c_int32), ("mbf", _f), ("bounds4", _f * 4), ("grid_w_inv", _f),
                ("grid_h_inv", _f), ("min_line_length_3d", _f), ("use_median_depth", ctypes.c_int32), ("median_fallback", _f)]


class RgbdFrameC(ctypes.Structure):     # plvs_rgbd_frame
    _fields_ = [("kp_cap", ctypes.c_int32), ("line_cap", ctypes.c_int32)] + \
               [(k, _vp) for k in ("kps", "kps_un", "desc", "u_right", "depth", "cell_start", "cell_items", "keylines", "keylines_un",
                                   "line_desc", "u_right_start", "depth_start", "u_right_end", "depth_end")] + \
               [(k, ctypes.c_int32) for k in ("n_kp", "mono_index", "n_lines", "n_items")] + [("median_depth", _f)]


L.plvs_hip_frame_rgbd_dev.argtypes = [_vp, _vp, _vp, _i, _i, _i, _vp, _i, ctypes.POINTER(RgbdCalib), ctypes.POINTER(RgbdFrameC), _vp]


def _depth_arg(depth):
    """-> (pointer, width, height, pitch in floats, on the device?, keep-alive)"""
    import numpy as np
    if isinstance(depth, torch.Tensor):
        assert depth.is_cuda and depth.dtype == torch.float32 and depth.dim() == 2 and depth.stride(1) == 1
        torch.cuda.current_stream().synchronize()
        return _vp(depth.data_ptr()), depth.shape[1], depth.shape[0], depth.stride(0), True, depth
    d = np.asarray(depth)
    assert d.dtype == np.float32 and d.ndim == 2
    if d.strides[1] != 4 or d.strides[0] % 4 or d.strides[0] < 4 * d.shape[1]:
        d = np.ascontiguousarray(d)
    return _vp(d.ctypes.data), d.shape[1], d.shape[0], d.strides[0] // 4, False, d


def _stereo_from_rgbd_dev(kps, kps_un, kl, kl_un, dp, w, h, pitch, K4, mbf, min_len):
    import numpy as np
    n, nl = len(kps), len(kl)
    out = [np.empty(n, np.float32) for _ in range(2)] + [np.empty(nl, np.float32) for _ in range(4)]
    _lib.check(L.plvs_hip_frame_stereo_from_rgbd_dev(_lib.np_ptr(kps), _lib.np_ptr(kps_un), n, _lib.np_ptr(kl), _lib.np_ptr(kl_un), nl,
                                                     dp, w, h, pitch, _lib.np_ptr(K4), float(mbf), float(min_len),
                                                     *[_lib.np_ptr(o) for o in out], _lib.current_stream_ptr()))
    return out


def ComputeStereoFromRGBD(kps, kps_un, depth, mbf):
    """Frame::ComputeStereoFromRGBD (src/Frame.cc:2251-2279) -> (mvuRight, mvDepth); -1 where the depth under the (distorted) key
    point is not > 0, and for a key point outside the image."""
    import numpy as np
    from .orb import KP_DTYPE
    kps, kps_un = np.ascontiguousarray(kps, KP_DTYPE), np.ascontiguousarray(kps_un, KP_DTYPE)
    assert len(kps) == len(kps_un)
    dp, w, h, pitch, on_dev, _keep = _depth_arg(depth)
    if on_dev:
        from .lines import KEYLINE_DTYPE
        none = np.zeros(0, KEYLINE_DTYPE)
        return tuple(_stereo_from_rgbd_dev(kps, kps_un, none, none, dp, w, h, pitch, None, mbf, 0.0)[:2])
    ur, z = np.empty(len(kps), np.float32), np.empty(len(kps), np.float32)
    _lib.check(L.plvs_hip_frame_compute_stereo_from_rgbd(_lib.np_ptr(kps), _lib.np_ptr(kps_un), len(kps), dp, w, h, pitch, float(mbf),
                                                         _lib.np_ptr(ur), _lib.np_ptr(z)))
    return ur, z


def ComputeStereoLinesFromRGBD(keylines, keylines_un, depth, K, mbf, min_line_length_3d=SK_MIN_LINE_LENGTH_3D):
    """Frame::ComputeStereoLinesFromRGBD (src/Frame.cc:2434-2674) on mvKeyLines / mvKeyLinesUn as UndistortKeyLines leaves them
    (same index) -> (mvuRightLineStart, mvDepthLineStart, mvuRightLineEnd, mvDepthLineEnd)."""
    import numpy as np
    from .lines import KEYLINE_DTYPE
    from .orb import KP_DTYPE
    kl, klu = np.ascontiguousarray(keylines, KEYLINE_DTYPE), np.ascontiguousarray(keylines_un, KEYLINE_DTYPE)
    assert len(kl) == len(klu)
    K4 = np.ascontiguousarray(K, np.float32).reshape(4)
    dp, w, h, pitch, on_dev, _keep = _depth_arg(depth)
    if on_dev:
        none = np.zeros(0, KP_DTYPE)
        return tuple(_stereo_from_rgbd_dev(none, none, kl, klu, dp, w, h, pitch, K4, mbf, min_line_length_3d)[2:])
    out = [np.empty(len(kl), np.float32) for _ in range(4)]
    _lib.check(L.plvs_hip_frame_compute_stereo_lines_from_rgbd(_lib.np_ptr(kl), _lib.np_ptr(klu), len(kl), dp, w, h, pitch, _lib.np_ptr(K4),
                                                               float(mbf), float(min_line_length_3d), *[_lib.np_ptr(o) for o in out]))
    return tuple(out)


def stereo_from_rgbd(kps, kps_un, keylines, keylines_un, depth, K, mbf, min_line_length_3d=SK_MIN_LINE_LENGTH_3D):
    """Both associations in one launch (plvs_hip_frame_stereo_from_rgbd_dev), depth: a float32 CUDA tensor ->
    (mvuRight, mvDepth, mvuRightLineStart, mvDepthLineStart, mvuRightLineEnd, mvDepthLineEnd).  Either set may be empty."""
    import numpy as np
    from .lines import KEYLINE_DTYPE
    from .orb import KP_DTYPE
    kps, kps_un = np.ascontiguousarray(kps, KP_DTYPE), np.ascontiguousarray(kps_un, KP_DTYPE)
    kl, klu = np.ascontiguousarray(keylines, KEYLINE_DTYPE), np.ascontiguousarray(keylines_un, KEYLINE_DTYPE)
    assert len(kps) == len(kps_un) and len(kl) == len(klu)
    dp, w, h, pitch, on_dev, _keep = _depth_arg(depth)
    assert on_dev, "stereo_from_rgbd reads the depth image in device memory"
    K4 = np.ascontiguousarray(K, np.float32).reshape(4)
    return tuple(_stereo_from_rgbd_dev(kps, kps_un, kl, klu, dp, w, h, pitch, K4, mbf, min_line_length_3d))


def ComputeSceneMedianDepth(depths, fallback=SK_FOV_CENTER_DISTANCE):
    """Frame::ComputeSceneMedianDepth (src/Frame.cc:2730-2751) over mvDepth."""
    import numpy as np
    d = np.ascontiguousarray(depths, np.float32).reshape(-1)
    m = _f()
    _lib.check(L.plvs_hip_frame_scene_median_depth(_lib.np_ptr(d), len(d), float(fallback), ctypes.byref(m)))
    return np.float32(m.value)


def rgbd_frame(orb: ORBextractor, lines, image: torch.Tensor, depth: torch.Tensor, K, dist, mbf, bounds, grid_w_inv, grid_h_inv,
               min_line_length_3d=SK_MIN_LINE_LENGTH_3D, use_median_depth=False, median_fallback=SK_FOV_CENTER_DISTANCE):
    """The RGB-D Frame constructor (src/Frame.cc:401-600) in one call: image (uint8) and depth (float32) are 2-D CUDA tensors of
    one size; lines = a LineExtractor or None; bounds = (mnMinX, mnMaxX, mnMinY, mnMaxY).  -> dict of what the Frame holds:
    mono_index, keys, keys_un, descriptors, u_right, depth, median_depth, keylines, keylines_un, line_descriptors,
    u_right_start, depth_start, u_right_end, depth_end, cell_start, cell_items."""
    import numpy as np
    from .lines import KEYLINE_DTYPE
    from .orb import KP_DTYPE
    assert image.is_cuda and image.dtype == torch.uint8 and image.dim() == 2 and image.stride(1) == 1
    dp, w, h, pitch, on_dev, _keep = _depth_arg(depth)
    assert on_dev and (h, w) == tuple(image.shape)
    K4, d, nd = _calib(K, dist)
    c = RgbdCalib()
    c.K4[:] = [float(x) for x in K4]
    for k in range(nd):
        c.dist[k] = float(d[k])
    c.ndist, c.mbf = nd, float(mbf)
    c.bounds4[:] = [float(x) for x in np.asarray(bounds, np.float32)[:4]]
    c.grid_w_inv, c.grid_h_inv, c.min_line_length_3d = float(grid_w_inv), float(grid_h_inv), float(min_line_length_3d)
    c.use_median_depth, c.median_fallback = int(bool(use_median_depth)), float(median_fallback)
    ncap, lcap = orb._cap, (lines._cap if lines is not None else 0)
    a = dict(kps=np.zeros(ncap, KP_DTYPE), kps_un=np.zeros(ncap, KP_DTYPE), desc=np.zeros((ncap, 32), np.uint8),
             u_right=np.zeros(ncap, np.float32), depth=np.zeros(ncap, np.float32), cell_start=np.zeros(64 * 48 + 1, np.int32),
             cell_items=np.zeros(ncap, np.int32))
    if lines is not None:
        a.update(keylines=np.zeros(lcap, KEYLINE_DTYPE), keylines_un=np.zeros(lcap, KEYLINE_DTYPE), line_desc=np.zeros((lcap, 32), np.uint8),
                 **{k: np.zeros(lcap, np.float32) for k in ("u_right_start", "depth_start", "u_right_end", "depth_end")})
    f = RgbdFrameC()
    f.kp_cap, f.line_cap = ncap, lcap
    for k, v in a.items():
        setattr(f, k, v.ctypes.data)
    _lib.check(L.plvs_hip_frame_rgbd_dev(orb._h, lines._h if lines is not None else None, _vp(image.data_ptr()), w, h, image.stride(0),
                                         dp, pitch, ctypes.byref(c), ctypes.byref(f), _lib.current_stream_ptr()))
    n, nl = f.n_kp, f.n_lines
    empty_l = np.zeros(0, np.float32)
    line = (lambda k: a[k][:nl].copy()) if lines is not None else (lambda k: empty_l.copy())
    return dict(mono_index=f.mono_index, keys=a["kps"][:n].copy(), keys_un=a["kps_un"][:n].copy(), descriptors=a["desc"][:n].copy(),
                u_right=a["u_right"][:n].copy(), depth=a["depth"][:n].copy(), median_depth=np.float32(f.median_depth),
                keylines=a["keylines"][:nl].copy() if lines is not None else np.zeros(0, KEYLINE_DTYPE),
                keylines_un=a["keylines_un"][:nl].copy() if lines is not None else np.zeros(0, KEYLINE_DTYPE),
                line_descriptors=a["line_desc"][:nl].copy() if lines is not None else np.zeros((0, 32), np.uint8),
                u_right_start=line("u_right_start"), depth_start=line("depth_start"), u_right_end=line("u_right_end"),
                depth_end=line("depth_end"), cell_start=a["cell_start"].copy(), cell_items=a["cell_items"][:f.n_items].copy())


# ---------------------------------------------------------------------------------------------- Frame glue, stereo
# What gives the lines of a stereo frame their depth (Frame::ComputeStereoLineMatches, src/Frame.cc:2008-2248, with
# LineMatcher::SearchStereoMatchesByKnn inside it: one launch) and the stereo constructor (:214-398) as one call.
SK_LINE_STEREO_MAX_DIST = 20.0    # Tracking::skLineStereoMaxDist (src/Tracking.cc:91)
TH_LOW_STEREO = 50                # LineMatcher::TH_LOW_STEREO (src/LineMatcher.cc:89)
STEREO_LINE_CAPACITY = 512        # lines per side of compute_stereo_line_matches
_LINE_MATCH_ARGS = [_vp, _vp, _i, _vp, _vp, _i, _vp, _i, _vp, _f, _f, _f, _f, _i, _i, _vp, _vp, _vp, _vp, _vp]
L.plvs_hip_frame_compute_stereo_line_matches.argtypes = _LINE_MATCH_ARGS + [_vp]
L.plvs_hip_frame_compute_stereo_line_matches_debug.argtypes = _LINE_MATCH_ARGS + [_vp, _vp]


def compute_stereo_line_matches(keylines_un, descriptors, keylines_right_un, descriptors_right, line_level_sigma2, K, mbf,
                                line_stereo_max_dist=SK_LINE_STEREO_MAX_DIST, min_line_length_3d=SK_MIN_LINE_LENGTH_3D, nn_ratio=0.7,
                                check_orientation=True, descriptor_dist=TH_LOW_STEREO, holders=False):
    """Frame::ComputeStereoLineMatches on mvKeyLinesUn / mLineDescriptors and their right twins (a rectified pair) ->
    (mvuRightLineStart, mvDepthLineStart, mvuRightLineEnd, mvDepthLineEnd, lines with depth).  nn_ratio / check_orientation =
    the LineMatcher(0.7) the reference builds.  holders=True appends the matcher stage's result: [n_right, 4] int32 = holding
    left line (-1 none), distance, valid after the rotation check, lowest passing left line that named it."""
    import numpy as np
    from .lines import KEYLINE_DTYPE
    kl, klr = np.ascontiguousarray(keylines_un, KEYLINE_DTYPE), np.ascontiguousarray(keylines_right_un, KEYLINE_DTYPE)
    d, dr = np.ascontiguousarray(descriptors, np.uint8).reshape(-1, 32), np.ascontiguousarray(descriptors_right, np.uint8).reshape(-1, 32)
    assert len(kl) == len(d) and len(klr) == len(dr)
    s2 = np.ascontiguousarray(line_level_sigma2, np.float32).reshape(-1)
    K4 = np.ascontiguousarray(K, np.float32).reshape(4)
    out = [np.empty(len(kl), np.float32) for _ in range(4)]
    ns = _i()
    args = (_lib.np_ptr(kl), _lib.np_ptr(d), len(kl), _lib.np_ptr(klr), _lib.np_ptr(dr), len(klr), _lib.np_ptr(s2), len(s2), _lib.np_ptr(K4),
            float(mbf), float(line_stereo_max_dist), float(min_line_length_3d), float(nn_ratio), int(bool(check_orientation)),
            int(descriptor_dist), *[_lib.np_ptr(o) for o in out], ctypes.byref(ns))
    if holders:
        h = np.full((max(len(klr), 1), 4), -1, np.int32)
        _lib.check(L.plvs_hip_frame_compute_stereo_line_matches_debug(*args, _lib.np_ptr(h), _lib.current_stream_ptr()))
        return (*out, ns.value, h[:len(klr)])
    _lib.check(L.plvs_hip_frame_compute_stereo_line_matches(*args, _lib.current_stream_ptr()))
    return (*out, ns.value)


class StereoCalib(ctypes.Structure):     # plvs_stereo_calib
    _fields_ = [("K4", _f * 4), ("dist", _f * 8), ("ndist", ctypes.c_int32), ("mbf", _f), ("bounds4", _f * 4), ("grid_w_inv", _f),
                ("grid_h_inv", _f), ("min_line_length_3d", _f), ("line_stereo_max_dist", _f), ("nn_ratio", _f),
                ("check_orientation", ctypes.c_int32), ("descriptor_dist", ctypes.c_int32), ("n_line_levels", ctypes.c_int32),
                ("line_level_sigma2", _vp)]


class StereoFrameC(ctypes.Structure):    # plvs_stereo_frame
    _fields_ = [(k, ctypes.c_int32) for k in ("kp_cap", "kp_right_cap", "line_cap", "line_right_cap")] + \
               [(k, _vp) for k in ("kps", "kps_un", "desc", "u_right", "depth", "cell_start", "cell_items", "kps_right", "desc_right",
                                   "keylines", "keylines_un", "line_desc", "u_right_start", "depth_start", "u_right_end", "depth_end",
                                   "keylines_right", "keylines_right_un", "line_desc_right")] + \
               [(k, ctypes.c_int32) for k in ("n_kp", "mono_index", "n_kp_right", "mono_index_right", "n_lines", "n_lines_right", "n_items",
                                              "n_stereo_points", "n_stereo_lines")]


L.plvs_hip_frame_stereo_dev.argtypes = [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, ctypes.POINTER(StereoCalib),
                                        ctypes.POINTER(StereoFrameC), _vp]


def frame_stereo(orb_left: ORBextractor, orb_right: ORBextractor, lines_left, lines_right, stereo, image_left: torch.Tensor,
                 image_right: torch.Tensor, K, dist, mbf, bounds, grid_w_inv, grid_h_inv, line_level_sigma2=None,
                 line_stereo_max_dist=SK_LINE_STEREO_MAX_DIST, min_line_length_3d=SK_MIN_LINE_LENGTH_3D, nn_ratio=0.7,
                 check_orientation=True, descriptor_dist=TH_LOW_STEREO):
    """The stereo Frame constructor (src/Frame.cc:214-398) in one call on a RECTIFIED pair (dist None or dist[0] == 0): two 2-D
    uint8 CUDA tensors of one size and stride; lines_left / lines_right = two LineExtractors or both None; stereo = the
    StereoMatcher made from orb_left and orb_right.  No bounds filter and no compaction of the lines (mvKeyLinesUn = mvKeyLines).
    -> dict of what the Frame holds: mono_index, keys, keys_un, descriptors, u_right, depth, keys_right, descriptors_right,
    keylines, keylines_un, line_descriptors, u_right_start, depth_start, u_right_end, depth_end, keylines_right,
    keylines_right_un, line_descriptors_right, cell_start, cell_items, n_stereo_points, n_stereo_lines."""
    import numpy as np
    from .lines import KEYLINE_DTYPE
    from .orb import KP_DTYPE
    for im in (image_left, image_right):
        assert im.is_cuda and im.dtype == torch.uint8 and im.dim() == 2 and im.stride(1) == 1
    assert image_left.shape == image_right.shape and image_left.stride(0) == image_right.stride(0)
    torch.cuda.current_stream().synchronize()
    h, w = image_left.shape
    K4, d, nd = _calib(K, dist)
    c = StereoCalib()
    c.K4[:] = [float(x) for x in K4]
    for k in range(min(nd, 8)):
        c.dist[k] = float(d[k])
    c.ndist, c.mbf = nd, float(mbf)
    c.bounds4[:] = [float(x) for x in np.asarray(bounds, np.float32)[:4]]
    c.grid_w_inv, c.grid_h_inv, c.min_line_length_3d = float(grid_w_inv), float(grid_h_inv), float(min_line_length_3d)
    c.line_stereo_max_dist, c.nn_ratio = float(line_stereo_max_dist), float(nn_ratio)
    c.check_orientation, c.descriptor_dist = int(bool(check_orientation)), int(descriptor_dist)
    s2 = None if line_level_sigma2 is None else np.ascontiguousarray(line_level_sigma2, np.float32).reshape(-1)
    c.n_line_levels, c.line_level_sigma2 = (0 if s2 is None else len(s2)), (None if s2 is None else s2.ctypes.data)
    with_lines = lines_left is not None
    ncap, rcap = orb_left._cap, orb_right._cap
    lcap, lrcap = (lines_left._cap, lines_right._cap) if with_lines else (0, 0)
    a = dict(kps=np.zeros(ncap, KP_DTYPE), kps_un=np.zeros(ncap, KP_DTYPE), desc=np.zeros((ncap, 32), np.uint8),
             u_right=np.zeros(ncap, np.float32), depth=np.zeros(ncap, np.float32), cell_start=np.zeros(64 * 48 + 1, np.int32),
             cell_items=np.zeros(ncap, np.int32), kps_right=np.zeros(rcap, KP_DTYPE), desc_right=np.zeros((rcap, 32), np.uint8))
    if with_lines:
        a.update(keylines=np.zeros(lcap, KEYLINE_DTYPE), keylines_un=np.zeros(lcap, KEYLINE_DTYPE), line_desc=np.zeros((lcap, 32), np.uint8),
                 keylines_right=np.zeros(lrcap, KEYLINE_DTYPE), keylines_right_un=np.zeros(lrcap, KEYLINE_DTYPE),
                 line_desc_right=np.zeros((lrcap, 32), np.uint8),
                 **{k: np.zeros(lcap, np.float32) for k in ("u_right_start", "depth_start", "u_right_end", "depth_end")})
    f = StereoFrameC()
    f.kp_cap, f.kp_right_cap, f.line_cap, f.line_right_cap = ncap, rcap, lcap, lrcap
    for k, v in a.items():
        setattr(f, k, v.ctypes.data)
    _lib.check(L.plvs_hip_frame_stereo_dev(orb_left._h, orb_right._h, lines_left._h if with_lines else None,
                                           lines_right._h if with_lines else None, stereo._h if stereo is not None else None,
                                           _vp(image_left.data_ptr()), _vp(image_right.data_ptr()), w, h, image_left.stride(0),
                                           ctypes.byref(c), ctypes.byref(f), _lib.current_stream_ptr()))
    n, nr, nl, nlr = f.n_kp, f.n_kp_right, f.n_lines, f.n_lines_right
    nlru = nlr if nl > 0 else 0           # mvKeyLinesRightUn is filled by UndistortKeyLines: only when left lines were found
    empty = dict(keylines=np.zeros(0, KEYLINE_DTYPE), line_desc=np.zeros((0, 32), np.uint8))      # without line extractors

    def take(k, m):
        if with_lines:
            return a[k][:m].copy()
        return empty.get(k.replace("_right", "").replace("_un", ""), np.zeros(0, np.float32)).copy()

    return dict(mono_index=f.mono_index, keys=a["kps"][:n].copy(), keys_un=a["kps_un"][:n].copy(), descriptors=a["desc"][:n].copy(),
                u_right=a["u_right"][:n].copy(), depth=a["depth"][:n].copy(), keys_right=a["kps_right"][:nr].copy(),
                descriptors_right=a["desc_right"][:nr].copy(), keylines=take("keylines", nl), keylines_un=take("keylines_un", nl),
                line_descriptors=take("line_desc", nl), u_right_start=take("u_right_start", nl), depth_start=take("depth_start", nl),
                u_right_end=take("u_right_end", nl), depth_end=take("depth_end", nl), keylines_right=take("keylines_right", nlr),
                keylines_right_un=take("keylines_right_un", nlru), line_descriptors_right=take("line_desc_right", nlr),
                cell_start=a["cell_start"].copy(), cell_items=a["cell_items"][:f.n_items].copy(),
                n_stereo_points=f.n_stereo_points, n_stereo_lines=f.n_stereo_lines)


# ---------------------------------------------------------------------------------------------- the local map (TrackLocalMap)
# Frame::isInFrustum over the local map points and lines (src/Frame.cc:955-1142, the loops of Tracking::SearchLocalPoints /
# SearchLocalLines) in one launch, and the two searches behind them in one call.
class TrackCameraC(ctypes.Structure):       # plvs_track_camera
    _fields_ = [("n_cameras", ctypes.c_int32), ("camera_model", ctypes.c_int32), ("K4", _vp), ("mbf", ctypes.c_float), ("bounds4", _vp),
                ("Rcw", _vp), ("tcw", _vp), ("Ow", _vp), ("viewing_cos_limit", ctypes.c_float), ("log_scale_factor", ctypes.c_float),
                ("n_levels", ctypes.c_int32), ("line_log_scale_factor", ctypes.c_float), ("n_line_levels", ctypes.c_int32)]


class TrackPointsC(ctypes.Structure):       # plvs_track_points
    _fields_ = [("m", ctypes.c_int32)] + [(k, _vp) for k in ("skip", "pos", "normal", "min_dist", "max_dist", "desc", "has_obs", "in_view",
                                                             "proj_x", "proj_y", "proj_xr", "track_depth", "level", "view_cos")]


class TrackLinesC(ctypes.Structure):        # plvs_track_lines
    _fields_ = [("m", ctypes.c_int32)] + [(k, _vp) for k in ("skip", "start", "end", "normal", "max_dist", "desc", "has_obs", "in_view",
                                                             "proj", "proj_xr", "level", "view_cos")]


PLVS_CAMERA_PINHOLE = 0
L.plvs_hip_frame_is_in_frustum.argtypes = [_vp] * 7
L.plvs_hip_frame_search_local_map.argtypes = ([_vp] * 5 + [ctypes.c_float, _i, ctypes.c_float, ctypes.c_float, _i] + [_vp] * 10)
L.plvs_hip_frame_track_test_flip.argtypes = [_i]
L.plvs_hip_frame_track_test_flip.restype = None


def _track_camera(cam):
    import numpy as np
    keep = [np.ascontiguousarray(cam[k], np.float32) for k in ("K4", "bounds4", "Rcw", "tcw", "Ow")]
    assert keep[0].size == 4 and keep[1].size == 4 and keep[2].size == 9 and keep[3].size == 3 and keep[4].size == 3
    c = TrackCameraC(int(cam.get("n_cameras", 1)), int(cam.get("camera_model", PLVS_CAMERA_PINHOLE)), _lib.np_ptr(keep[0]), float(cam["mbf"]),
                     _lib.np_ptr(keep[1]), _lib.np_ptr(keep[2]), _lib.np_ptr(keep[3]), _lib.np_ptr(keep[4]), float(cam["viewing_cos_limit"]),
                     float(cam["log_scale_factor"]), int(cam["n_levels"]), float(cam["line_log_scale_factor"]), int(cam["n_line_levels"]))
    return c, keep


def _track_points(points):
    import numpy as np
    f, u8 = (lambda a: np.ascontiguousarray(a, np.float32)), (lambda a: None if a is None else np.ascontiguousarray(a, np.uint8))
    m = len(points["skip"])
    ins = [u8(points["skip"]), f(points["pos"]), f(points["normal"]), f(points["min_dist"]), f(points["max_dist"]), u8(points.get("desc")),
           u8(points.get("has_obs"))]
    out = dict(in_view=np.zeros(m, np.uint8), proj_x=np.zeros(m, np.float32), proj_y=np.zeros(m, np.float32), proj_xr=np.zeros(m, np.float32),
               track_depth=np.zeros(m, np.float32), level=np.zeros(m, np.int32), view_cos=np.zeros(m, np.float32))
    c = TrackPointsC(m, *[_lib.np_ptr(a) for a in ins], *[_lib.np_ptr(out[k]) for k in ("in_view", "proj_x", "proj_y", "proj_xr", "track_depth",
                                                                                       "level", "view_cos")])
    return c, ins, out


def _track_lines(lines):
    import numpy as np
    f, u8 = (lambda a: np.ascontiguousarray(a, np.float32)), (lambda a: None if a is None else np.ascontiguousarray(a, np.uint8))
    m = len(lines["skip"])
    ins = [u8(lines["skip"]), f(lines["start"]), f(lines["end"]), f(lines["normal"]), f(lines["max_dist"]), u8(lines.get("desc")),
           u8(lines.get("has_obs"))]
    out = dict(in_view=np.zeros(m, np.uint8), proj=np.zeros((m, 6), np.float32), proj_xr=np.zeros((m, 2), np.float32),
               level=np.zeros(m, np.int32), view_cos=np.zeros(m, np.float32))
    c = TrackLinesC(m, *[_lib.np_ptr(a) for a in ins], *[_lib.np_ptr(out[k]) for k in ("in_view", "proj", "proj_xr", "level", "view_cos")])
    return c, ins, out


_STATS = ("ambiguous_points", "ambiguous_lines", "levels_changed", "window_launches")


def is_in_frustum(cam, points=None, lines=None):
    """Frame::isInFrustum over the local map.  cam: dict(K4, mbf, bounds4, Rcw [9, as Eigen::Matrix3f holds mRcw], tcw, Ow,
    viewing_cos_limit, log_scale_factor, n_levels, line_log_scale_factor, n_line_levels); points: dict(skip, pos, normal,
    min_dist, max_dist) or None; lines: dict(skip, start, end, normal, max_dist) or None.
    -> dict(points=dict(in_view, proj_x, proj_y, proj_xr, track_depth, level, view_cos) | None, lines=dict(in_view, proj [m, 6],
    proj_xr [m, 2], level, view_cos) | None, n_in_view_points, n_in_view_lines (the reference's nToMatch), stats)."""
    import numpy as np
    c, keep = _track_camera(cam)
    pc, pk, po = _track_points(points) if points is not None else (None, None, None)
    lc, lk, lo = _track_lines(lines) if lines is not None else (None, None, None)
    nv, nvl, stats = _i(), _i(), np.zeros(4, np.int32)
    _lib.check(L.plvs_hip_frame_is_in_frustum(ctypes.byref(c), ctypes.byref(pc) if pc else None, ctypes.byref(lc) if lc else None,
                                              ctypes.byref(nv), ctypes.byref(nvl), _lib.np_ptr(stats), None))
    return dict(points=po, lines=lo, n_in_view_points=nv.value, n_in_view_lines=nvl.value, stats=dict(zip(_STATS, (int(s) for s in stats))))


def search_local_map(cam, frame_view, line_view, points, lines=None, th=1.0, far_points=False, th_far=50.0, nn_ratio=0.8, larger_search=False,
                     occupied_points=None, occupied_lines=None):
    """The frustum loops, then ORBmatcher::SearchByProjection(F, vpMapPoints, th, bFarPoints, thFarPoints) and
    LineMatcher::SearchByProjection(F, vpMapLines, bLargerSearch), with one device wait on the common path.  frame_view: an
    orbmatcher.FrameView; line_view: what linematcher.line_frame_view returns, or None (no lines); points / lines as in
    is_in_frustum, plus desc and (optionally) has_obs.  -> is_in_frustum's dict plus assigned_points, nmatches_points,
    assigned_lines, nmatches_lines."""
    import numpy as np
    c, keep = _track_camera(cam)
    fc = frame_view.as_c()
    pc, pk, po = _track_points(points)
    lc, lk, lo = _track_lines(lines) if lines is not None else (None, None, None)
    lv = line_view[0] if line_view is not None else None
    u8 = lambda a: None if a is None else np.ascontiguousarray(a, np.uint8)
    occ_p, occ_l = u8(occupied_points), u8(occupied_lines)
    ap = np.full(max(fc.n, 1), -7, np.int32)
    al = np.full(max(lv.n if lv is not None else 0, 1), -7, np.int32)
    np_, nl_, nv, nvl, stats = _i(), _i(), _i(), _i(), np.zeros(4, np.int32)
    _lib.check(L.plvs_hip_frame_search_local_map(ctypes.byref(c), ctypes.byref(fc), ctypes.byref(lv) if lv is not None else None, ctypes.byref(pc),
                                                 ctypes.byref(lc) if lc else None, float(th), int(far_points), float(th_far), float(nn_ratio),
                                                 int(larger_search), _lib.np_ptr(occ_p), _lib.np_ptr(occ_l), _lib.np_ptr(ap), ctypes.byref(np_),
                                                 _lib.np_ptr(al), ctypes.byref(nl_), ctypes.byref(nv), ctypes.byref(nvl), _lib.np_ptr(stats), None))
    return dict(points=po, lines=lo, n_in_view_points=nv.value, n_in_view_lines=nvl.value, stats=dict(zip(_STATS, (int(s) for s in stats))),
                assigned_points=ap[:fc.n], nmatches_points=np_.value, assigned_lines=al[:lv.n] if lv is not None else al[:0],
                nmatches_lines=nl_.value)


def track_test_flip(point_index=-1):
    """Test hook: see plvs_hip_frame_track_test_flip."""
    L.plvs_hip_frame_track_test_flip(int(point_index))


# ---------------------------------------------------------------------------------------------- the last frame (TrackWithMotionModel)
# The search of Tracking::TrackWithMotionModel (src/Tracking.cc:3615-3664) in one call: the projection of the last frame's map
# points and lines on the device, the two SearchByProjection(CurrentFrame, LastFrame, ...) behind it, the retry rules.
class MotionPosesC(ctypes.Structure):       # plvs_motion_poses
    _fields_ = [("n_cameras", ctypes.c_int32), ("camera_model", ctypes.c_int32), ("mono", ctypes.c_int32), ("q_cw", _vp), ("tcw", _vp),
                ("Rcw", _vp), ("Ow", _vp), ("q_lw", _vp), ("tlw", _vp), ("mb", ctypes.c_float), ("mbf", ctypes.c_float), ("bounds4", _vp),
                ("K4", _vp), ("K4_linear", _vp)]


class MotionPointsC(ctypes.Structure):      # plvs_motion_points
    _fields_ = [("n", ctypes.c_int32)] + [(k, _vp) for k in ("valid", "pos", "octave", "angle", "desc", "has_obs", "proj_valid", "u", "v", "invz")]


class MotionLinesC(ctypes.Structure):       # plvs_motion_lines
    _fields_ = [("n", ctypes.c_int32)] + [(k, _vp) for k in ("valid", "start", "end", "max_dist", "octave", "angle", "desc", "has_obs",
                                                             "proj_valid", "proj6")]


class MotionPolicyC(ctypes.Structure):      # plvs_motion_policy
    _fields_ = [("th", ctypes.c_float), ("nn_ratio_points", ctypes.c_float), ("nn_ratio_lines", ctypes.c_float),
                ("check_orientation", ctypes.c_int32), ("min_point_matches", ctypes.c_int32), ("min_line_matches", ctypes.c_int32)]


class MotionResultC(ctypes.Structure):      # plvs_motion_result
    _fields_ = [("nmatches_points", ctypes.c_int32), ("nmatches_lines", ctypes.c_int32), ("forward", ctypes.c_int32), ("backward", ctypes.c_int32),
                ("th_used", ctypes.c_float), ("larger_line_search_used", ctypes.c_int32)]


L.plvs_hip_frame_search_last_frame.argtypes = [_vp] * 14
_MOTION_STATS = ("window_launches", "point_retries", "line_retries", "candidate_spills")


def search_last_frame(poses, frame_view, cur_angle, line_view, points, lines=None, th=15.0, nn_ratio_points=0.9, nn_ratio_lines=0.9,
                      check_orientation=True, min_point_matches=0, min_line_matches=0, occupied_points=None, occupied_lines=None):
    """ORBmatcher::SearchByProjection(CurrentFrame, LastFrame, th, bMono) and LineMatcher::SearchByProjection(CurrentFrame,
    LastFrame, bLargerSearch, bMono) with the projection of the last frame's map points and lines on the device; with
    min_point_matches = 20 and min_line_matches = 10 the retry rules of Tracking::TrackWithMotionModel.  poses: dict(q_cw [x, y, z,
    w], tcw, Rcw [9, as Eigen::Matrix3f holds mRcw], Ow, q_lw, tlw, mb, mbf, bounds4, K4, K4_linear (optional), mono, n_cameras
    (optional), camera_model (optional)); frame_view: an orbmatcher.FrameView; cur_angle: mvKeysUn[i].angle; line_view: what
    linematcher.line_frame_view returns, or None; points: dict(valid, pos, octave, angle, desc, has_obs (optional)) — None entries
    reach the library as NULL —; lines: dict(valid, start, end, max_dist, octave, angle, desc, has_obs (optional)) or None.
    -> dict(assigned_points, nmatches_points, assigned_lines, nmatches_lines, forward, backward, th_used,
    larger_line_search_used, proj_valid_points, u, v, invz, proj_valid_lines, proj6, stats)."""
    import numpy as np
    f = lambda a: None if a is None else np.ascontiguousarray(a, np.float32)
    u8 = lambda a: None if a is None else np.ascontiguousarray(a, np.uint8)
    i32 = lambda a: None if a is None else np.ascontiguousarray(a, np.int32)
    keep = [f(poses.get(k)) for k in ("q_cw", "tcw", "Rcw", "Ow", "q_lw", "tlw", "bounds4", "K4", "K4_linear")]
    pc = MotionPosesC(int(poses.get("n_cameras", 1)), int(poses.get("camera_model", PLVS_CAMERA_PINHOLE)), int(bool(poses.get("mono", 0))),
                      *[_lib.np_ptr(a) for a in keep[:6]], float(poses["mb"]), float(poses["mbf"]), *[_lib.np_ptr(a) for a in keep[6:]])
    fc = frame_view.as_c()
    ang = f(cur_angle)
    n = len(points["valid"])
    pin = [u8(points["valid"]), f(points["pos"]), i32(points["octave"]), f(points["angle"]), u8(points["desc"]), u8(points.get("has_obs"))]
    pout = dict(proj_valid=np.zeros(n, np.uint8), u=np.zeros(n, np.float32), v=np.zeros(n, np.float32), invz=np.zeros(n, np.float32))
    ptc = MotionPointsC(n, *[_lib.np_ptr(a) for a in pin], *[_lib.np_ptr(pout[k]) for k in ("proj_valid", "u", "v", "invz")])
    lc, lin, lout = None, None, dict(proj_valid=np.zeros(0, np.uint8), proj6=np.zeros((0, 6), np.float32))
    if lines is not None:
        nl = len(lines["valid"])
        lin = [u8(lines["valid"]), f(lines["start"]), f(lines["end"]), f(lines["max_dist"]), i32(lines["octave"]), f(lines["angle"]),
               u8(lines["desc"]), u8(lines.get("has_obs"))]
        lout = dict(proj_valid=np.zeros(nl, np.uint8), proj6=np.zeros((nl, 6), np.float32))
        lc = MotionLinesC(nl, *[_lib.np_ptr(a) for a in lin], _lib.np_ptr(lout["proj_valid"]), _lib.np_ptr(lout["proj6"]))
    lv = line_view[0] if line_view is not None else None
    occ_p, occ_l = u8(occupied_points), u8(occupied_lines)
    ap = np.full(max(fc.n, 1), -7, np.int32)
    al = np.full(max(lv.n if lv is not None else 0, 1), -7, np.int32)
    pol = MotionPolicyC(float(th), float(nn_ratio_points), float(nn_ratio_lines), int(bool(check_orientation)), int(min_point_matches),
                        int(min_line_matches))
    res, stats = MotionResultC(), np.zeros(4, np.int32)
    _lib.check(L.plvs_hip_frame_search_last_frame(ctypes.byref(pc), ctypes.byref(fc), _lib.np_ptr(ang), ctypes.byref(lv) if lv is not None else None,
                                                  ctypes.byref(ptc), ctypes.byref(lc) if lc is not None else None, ctypes.byref(pol),
                                                  _lib.np_ptr(occ_p), _lib.np_ptr(occ_l), _lib.np_ptr(ap), _lib.np_ptr(al), ctypes.byref(res),
                                                  _lib.np_ptr(stats), None))
    return dict(assigned_points=ap[:fc.n], nmatches_points=res.nmatches_points, assigned_lines=al[:lv.n] if lv is not None else al[:0],
                nmatches_lines=res.nmatches_lines, forward=res.forward, backward=res.backward, th_used=res.th_used,
                larger_line_search_used=res.larger_line_search_used, proj_valid_points=pout["proj_valid"], u=pout["u"], v=pout["v"],
                invz=pout["invz"], proj_valid_lines=lout["proj_valid"], proj6=lout["proj6"], stats=dict(zip(_MOTION_STATS, (int(s) for s in stats))))
