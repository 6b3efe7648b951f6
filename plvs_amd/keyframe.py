"""Key frames resident in HBM (include/plvs_hip.h: plvs_keyframe) and the Fuse searches of LocalMapping::SearchInNeighbors over them.

    kf = ResidentKeyFrame(points=FuseKeyFrame(...), lines=LineFuseKeyFrame(...))     # once, where the KeyFrame constructor ends
    out = fuse_search_kf([kf, ...], [KeyFramePose(q_cw, Rcw, tcw, Ow), ...], points, th, skip)
    kf.close()                                                                       # with the key frame, or on SetBadFlag

A handle holds what the constructor fixes; the pose travels with each call.  Outputs are those of ORBmatcher.FuseSearch /
LineMatcher.FuseSearch / FuseSearchPointsAndLines, with one more entry in stats: the bytes of the call's copy in.

The Sim3 Fuse searches of LoopClosing::SearchAndFuse (loop_fuse_search_kf, line_loop_fuse_search_kf,
loop_fuse_search_points_and_lines_kf) take the same handles and a Sim3Pose per key frame: the caller's own decomposition of Scw.

ORBmatcher::SearchByBoW over handles made with a KeyFrameBow (search_by_bow_kf: one key frame against K key frames, loop detection's
first stage; search_by_bow_frame_kf: K key frames against one BowFrame, relocalisation), each one call."""
import ctypes
from dataclasses import dataclass

import numpy as np

from . import _lib
from .linematcher import FuseLines, LineFuseKeyFrame, _fuse_outputs  # noqa: F401
from .orbmatcher import FeatureVector, FuseKeyFrame, FusePoints, _FeatVecC  # noqa: F401

_vp, _i, _f = ctypes.c_void_p, ctypes.c_int, ctypes.c_float
HOST_ONLY = 1
INFO = ("n_points", "n_lines", "device_bytes", "host_bytes", "flags", "device")
BOW_INFO = ("nodes", "listed", "longest", "device_bytes")


class _PoseC(ctypes.Structure):
    _fields_ = [("q_cw", _f * 4), ("Rcw", _f * 9), ("tcw", _f * 3), ("Ow", _f * 3)]


@dataclass
class KeyFramePose:
    """GetPose() / GetCameraCenter() at the time of the call."""
    q_cw: np.ndarray      # unit_quaternion().coeffs(): x, y, z, w (the point search's projection); None: zeros
    Rcw: np.ndarray       # rotationMatrix() in Eigen's layout: 9, column-major (the line search's); None: zeros
    tcw: np.ndarray
    Ow: np.ndarray

    def as_c(self):
        f = lambda a, n: (_f * n)(*(np.zeros(n, np.float32) if a is None else np.asarray(a, np.float32).reshape(n)).tolist())
        return _PoseC(f(self.q_cw, 4), f(self.Rcw, 9), f(self.tcw, 3), f(self.Ow, 3))


class _Sim3PoseC(ctypes.Structure):
    _fields_ = [("q_cw", _f * 4), ("Rcw", _f * 9), ("tcw", _f * 3), ("Ow_points", _f * 3), ("Ow_lines", _f * 3)]


@dataclass
class Sim3Pose:
    """plvs_keyframe_sim3_pose: Scw as the two Sim3 Fuse overloads decompose it, by the caller's own Sophus / Eigen."""
    q_cw: np.ndarray        # SE3f(Scw.rotationMatrix(), Scw.translation() / Scw.scale()).unit_quaternion().coeffs(); None: zeros
    Rcw: np.ndarray         # Scw.rotationMatrix(), 9, column-major; None: zeros
    tcw: np.ndarray         # Scw.translation() / Scw.scale()
    Ow_points: np.ndarray   # Tcw.inverse().translation(); None: zeros
    Ow_lines: np.ndarray    # -Rcw.transpose() * tcw; None: zeros

    def as_c(self):
        f = lambda a, n: (_f * n)(*(np.zeros(n, np.float32) if a is None else np.asarray(a, np.float32).reshape(n)).tolist())
        return _Sim3PoseC(f(self.q_cw, 4), f(self.Rcw, 9), f(self.tcw, 3), f(self.Ow_points, 3), f(self.Ow_lines, 3))


def pose_of(points=None, lines=None):
    """The pose a FuseKeyFrame and / or a LineFuseKeyFrame of the same key frame carry."""
    src = points if points is not None else lines
    return KeyFramePose(None if points is None else points.q_cw, None if lines is None else lines.Rcw, src.tcw, src.Ow)


class _KeyFrameBowC(ctypes.Structure):
    _fields_ = [("vec", _FeatVecC), ("angle", _vp)]


@dataclass
class KeyFrameBow:
    """plvs_keyframe_bow: what KeyFrame::ComputeBoW fixes of a key frame."""
    vec: FeatureVector    # pKF->mFeatVec
    angle: np.ndarray     # pKF->mvKeysUn[i].angle, degrees; None: a NULL angle (refused)

    def as_c(self):
        self._angle = None if self.angle is None else np.ascontiguousarray(self.angle, np.float32)
        return _KeyFrameBowC(self.vec.as_c(), _lib.np_ptr(self._angle))


class ResidentKeyFrame:
    """plvs_hip_keyframe_create / plvs_hip_keyframe_create_bow: a deep copy of `points` and / or `lines` (their pose fields are not
    read), with both grids, and of `bow` (a KeyFrameBow; needs points), on the host and — unless host_only — in one device allocation."""

    def __init__(self, points=None, lines=None, host_only=False, bow=None):
        self._h = _vp()
        pc = None if points is None else points.as_c()
        lc = None if lines is None else lines.as_c()
        if pc is not None:
            pc.q_cw = pc.tcw = pc.Ow = None      # the pose is the call's: create does not read these
        if lc is not None:
            lc.Rcw = lc.tcw = lc.Ow = None
        args = [None if pc is None else ctypes.byref(pc), None if lc is None else ctypes.byref(lc)]
        if bow is None:
            f = _lib.lib.plvs_hip_keyframe_create
            f.argtypes = [_vp, _vp, ctypes.c_uint32, _vp]
        else:
            bc = bow.as_c()
            args.append(ctypes.byref(bc))
            f = _lib.lib.plvs_hip_keyframe_create_bow
            f.argtypes = [_vp, _vp, _vp, ctypes.c_uint32, _vp]
        _lib.check(f(*args, HOST_ONLY if host_only else 0, ctypes.byref(self._h)))

    @property
    def handle(self):
        if not self._h:
            raise ValueError("the key frame handle is closed")
        return self._h.value

    def info(self):
        out = np.zeros(6, np.int64)
        f = _lib.lib.plvs_hip_keyframe_info
        f.argtypes = [_vp, _vp]
        _lib.check(f(self.handle, _lib.np_ptr(out)))
        return dict(zip(INFO, out.tolist()))

    def bow_info(self):
        out = np.zeros(4, np.int64)
        f = _lib.lib.plvs_hip_keyframe_bow_info
        f.argtypes = [_vp, _vp]
        _lib.check(f(self.handle, _lib.np_ptr(out)))
        return dict(zip(BOW_INFO, out.tolist()))

    def close(self):
        if self._h:
            f = _lib.lib.plvs_hip_keyframe_destroy
            f.argtypes = [_vp]
            h, self._h = self._h, _vp()
            _lib.check(f(h))

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _lists(key_frames, poses):
    K = len(key_frames)
    assert len(poses) == K
    hs = (_vp * max(K, 1))(*[None if kf is None else kf.handle for kf in key_frames])
    ps = ((_Sim3PoseC if poses and isinstance(poses[0], Sim3Pose) else _PoseC) * max(K, 1))(*[p.as_c() for p in poses])
    return K, hs, ps


def _stats4(out):
    return out[:3] + (np.full(4, -1, np.int32),)


def _single(name, key_frames, poses, items, th, skip, host, stream, want_reached, outputs):
    K, hs, ps = _lists(key_frames, poses)
    ic = items.as_c()
    M = ic.m
    sk = None if skip is None else np.ascontiguousarray(skip, np.uint8).reshape(K, M)
    best_idx, best_dist, reached, stats = _stats4(_fuse_outputs(K, M, outputs, want_reached))
    args = [hs if K else None, ps if K else None, K, ctypes.byref(ic), _lib.np_ptr(sk), th, _lib.np_ptr(best_idx), _lib.np_ptr(best_dist),
            _lib.np_ptr(reached), _lib.np_ptr(stats)]
    f = getattr(_lib.lib, name + ("_host" if host else ""))
    f.argtypes = [_vp, _vp, _i, _vp, _vp, _f, _vp, _vp, _vp, _vp] + ([] if host else [_vp])
    if not host:
        args.append(stream)
    _lib.check(f(*args))
    return dict(best_idx=best_idx, best_dist=best_dist, reached=reached, stats=stats)


def fuse_search_kf(key_frames, poses, points, th=3.0, skip=None, host=False, stream=None, want_reached=True, outputs=True):
    """ORBmatcher.FuseSearch over resident key frames (plvs_hip_orb_fuse_search_kf / _kf_host): key frame k = (key_frames[k],
    poses[k]).  -> dict(best_idx [K,M], best_dist [K,M], reached [K,M], stats [4])."""
    return _single("plvs_hip_orb_fuse_search_kf", key_frames, poses, points, th, skip, host, stream, want_reached, outputs)


def line_fuse_search_kf(key_frames, poses, lines, th=3.0, skip=None, host=False, stream=None, want_reached=True, outputs=True):
    """LineMatcher.FuseSearch over resident key frames (plvs_hip_line_fuse_search_kf / _kf_host)."""
    return _single("plvs_hip_line_fuse_search_kf", key_frames, poses, lines, th, skip, host, stream, want_reached, outputs)


def fuse_search_points_and_lines_kf(key_frames, poses, points=None, th_points=3.0, skip_points=None, lines=None, th_lines=3.0,
                                    skip_lines=None, stream=None, _name="plvs_hip_fuse_search_points_and_lines_kf"):
    """FuseSearchPointsAndLines over ONE list of resident key frames (plvs_hip_fuse_search_points_and_lines_kf).
    -> (points' dict or None, lines' dict or None, stats [3]: launches, waits, bytes of the copy in)."""
    K, hs, ps = _lists(key_frames, poses)
    pc = lc = psk = lsk = None
    p_out = l_out = (None, None, None, None)
    if points is not None:
        pc = points.as_c()
        psk = None if skip_points is None else np.ascontiguousarray(skip_points, np.uint8).reshape(K, pc.m)
        p_out = _stats4(_fuse_outputs(K, pc.m, True, True))
    if lines is not None:
        lc = lines.as_c()
        lsk = None if skip_lines is None else np.ascontiguousarray(skip_lines, np.uint8).reshape(K, lc.m)
        l_out = _stats4(_fuse_outputs(K, lc.m, True, True))
    stats = np.full(3, -1, np.int32)
    f = getattr(_lib.lib, _name)
    f.argtypes = [_vp, _vp, _i, _vp, _vp, _f, _vp, _vp, _vp, _vp, _vp, _vp, _f, _vp, _vp, _vp, _vp, _vp, _vp]
    _lib.check(f(hs if K else None, ps if K else None, K, None if pc is None else ctypes.byref(pc), _lib.np_ptr(psk), th_points,
                 *[_lib.np_ptr(a) for a in p_out], None if lc is None else ctypes.byref(lc), _lib.np_ptr(lsk), th_lines,
                 *[_lib.np_ptr(a) for a in l_out], _lib.np_ptr(stats), stream))
    as_dict = lambda o: dict(best_idx=o[0], best_dist=o[1], reached=o[2], stats=o[3])
    return (None if points is None else as_dict(p_out)), (None if lines is None else as_dict(l_out)), stats


def loop_fuse_search_kf(key_frames, sim3_poses, points, th=4.0, skip=None, host=False, stream=None, want_reached=True, outputs=True):
    """The search of ORBmatcher::Fuse(pKF, Scw, vpPoints, th, vpReplacePoint) over resident key frames
    (plvs_hip_orb_loop_fuse_search_kf / _kf_host): key frame k = (key_frames[k], sim3_poses[k]), a Sim3Pose each.
    -> dict(best_idx [K,M], best_dist [K,M], reached [K,M], stats [4])."""
    return _single("plvs_hip_orb_loop_fuse_search_kf", key_frames, sim3_poses, points, th, skip, host, stream, want_reached, outputs)


def line_loop_fuse_search_kf(key_frames, sim3_poses, lines, th=4.0, skip=None, host=False, stream=None, want_reached=True, outputs=True):
    """The search of LineMatcher::Fuse(pKF, Scw, vpLines, th, vpReplaceLine) over resident key frames
    (plvs_hip_line_loop_fuse_search_kf / _kf_host)."""
    return _single("plvs_hip_line_loop_fuse_search_kf", key_frames, sim3_poses, lines, th, skip, host, stream, want_reached, outputs)


def loop_fuse_search_points_and_lines_kf(key_frames, sim3_poses, points=None, th_points=4.0, skip_points=None, lines=None, th_lines=4.0,
                                         skip_lines=None, stream=None):
    """Both Sim3 searches over ONE list of resident key frames in one call (plvs_hip_loop_fuse_search_points_and_lines_kf).
    -> (points' dict or None, lines' dict or None, stats [3]: launches, waits, bytes of the copy in)."""
    return fuse_search_points_and_lines_kf(key_frames, sim3_poses, points, th_points, skip_points, lines, th_lines, skip_lines, stream,
                                           _name="plvs_hip_loop_fuse_search_points_and_lines_kf")


def loop_fuse_test_layout(mode):
    """plvs_hip_loop_fuse_test_layout: 0 = the sieve (default), 1 = a wave per pair, for the calling thread's later Sim3 point searches."""
    f = _lib.lib.plvs_hip_loop_fuse_test_layout
    f.argtypes = [_i]
    f.restype = None
    f(mode)


# ---- loop detection: the SearchByProjection(pKF, Scw, ...) overloads
PROJECT_CAMERA, PROJECT_INVZ = 0, 1


def _occupied(occupied, K):
    """-> (the const uint8_t* const* argument, what keeps its arrays alive).  occupied: None, or K entries, each None or n_k bytes."""
    if occupied is None:
        return None, None
    assert len(occupied) == K
    keep = [None if o is None else np.ascontiguousarray(o, np.uint8) for o in occupied]
    return (_vp * max(K, 1))(*[None if o is None else o.ctypes.data for o in keep]), keep


def _loop_search_outputs(K, M, want_reached):
    return (np.full((K, M), -2, np.int32), np.full((K, M), -2, np.int32), np.full((K, M), 255, np.uint8) if want_reached else None,
            np.full(K, -1, np.int32), np.full(5, -1, np.int32))


def _loop_search(name, key_frames, sim3_poses, items, th, ratio_hamming, projection, skip, occupied, host, stream, want_reached):
    K, hs, ps = _lists(key_frames, sim3_poses)
    ic = items.as_c()
    M = ic.m
    sk = None if skip is None else np.ascontiguousarray(skip, np.uint8).reshape(K, M)
    occ, keep = _occupied(occupied, K)
    match_idx, match_dist, reached, nmatches, stats = _loop_search_outputs(K, M, want_reached)
    args = [hs if K else None, ps if K else None, K, ctypes.byref(ic), _lib.np_ptr(sk), occ, th, ratio_hamming]
    types = [_vp, _vp, _i, _vp, _vp, _vp, _f, _f]
    if projection is not None:
        args.append(projection)
        types.append(_i)
    args += [_lib.np_ptr(match_idx), _lib.np_ptr(match_dist), _lib.np_ptr(reached), _lib.np_ptr(nmatches), _lib.np_ptr(stats)]
    types += [_vp] * 5
    if not host:
        args.append(stream)
        types.append(_vp)
    f = getattr(_lib.lib, name + ("_host" if host else ""))
    f.argtypes = types
    _lib.check(f(*args))
    return dict(match_idx=match_idx, match_dist=match_dist, reached=reached, nmatches=nmatches, stats=stats)


def loop_search_by_projection_kf(key_frames, sim3_poses, points, th=8.0, ratio_hamming=1.5, projection=PROJECT_CAMERA, skip=None,
                                 occupied=None, host=False, stream=None, want_reached=True):
    """ORBmatcher::SearchByProjection(pKF, Scw, vpPoints, vpMatched, th, ratioHamming) (projection = PROJECT_CAMERA) or its overload with
    vpPointsKFs / vpMatchedKF (PROJECT_INVZ) over resident key frames (plvs_hip_orb_loop_search_by_projection_kf / _kf_host): key frame
    k = (key_frames[k], sim3_poses[k]), ONE list of points.  occupied[k][j] != 0: vpMatched[j] of key frame k is not null on entry.
    -> dict(match_idx [K,M], match_dist [K,M], reached [K,M], nmatches [K], stats [5])."""
    return _loop_search("plvs_hip_orb_loop_search_by_projection_kf", key_frames, sim3_poses, points, th, ratio_hamming, projection, skip,
                        occupied, host, stream, want_reached)


def line_loop_search_by_projection_kf(key_frames, sim3_poses, lines, th=8.0, ratio_hamming=1.5, skip=None, occupied=None, host=False,
                                      stream=None, want_reached=True):
    """LineMatcher::SearchByProjection(pKF, Scw, vpLines, vpMatched, th, ratioHamming) and its overload with vpLinesKFs / vpMatchedKF
    (one projection serves both) over resident key frames (plvs_hip_line_loop_search_by_projection_kf / _kf_host).
    -> dict(match_idx [K,M], match_dist [K,M], reached [K,M], nmatches [K], stats [5])."""
    return _loop_search("plvs_hip_line_loop_search_by_projection_kf", key_frames, sim3_poses, lines, th, ratio_hamming, None, skip, occupied,
                        host, stream, want_reached)


def loop_search_by_projection_points_and_lines_kf(key_frames, sim3_poses, points=None, th_points=8.0, ratio_hamming_points=1.5,
                                                  projection=PROJECT_CAMERA, skip_points=None, occupied_points=None, lines=None, th_lines=8.0,
                                                  ratio_hamming_lines=1.5, skip_lines=None, occupied_lines=None, stream=None):
    """Both searches over ONE list of resident key frames in one call (plvs_hip_loop_search_by_projection_points_and_lines_kf).
    -> (points' dict or None, lines' dict or None, stats [3]: launches, waits, bytes of the copy in)."""
    K, hs, ps = _lists(key_frames, sim3_poses)
    pc = lc = psk = lsk = pocc = locc = None
    p_out = l_out = (None,) * 5
    if points is not None:
        pc = points.as_c()
        psk = None if skip_points is None else np.ascontiguousarray(skip_points, np.uint8).reshape(K, pc.m)
        pocc, pkeep = _occupied(occupied_points, K)
        p_out = _loop_search_outputs(K, pc.m, True)
    if lines is not None:
        lc = lines.as_c()
        lsk = None if skip_lines is None else np.ascontiguousarray(skip_lines, np.uint8).reshape(K, lc.m)
        locc, lkeep = _occupied(occupied_lines, K)
        l_out = _loop_search_outputs(K, lc.m, True)
    stats = np.full(3, -1, np.int32)
    f = _lib.lib.plvs_hip_loop_search_by_projection_points_and_lines_kf
    f.argtypes = [_vp, _vp, _i, _vp, _vp, _vp, _f, _f, _i] + [_vp] * 5 + [_vp, _vp, _vp, _f, _f] + [_vp] * 5 + [_vp, _vp]
    _lib.check(f(hs if K else None, ps if K else None, K, None if pc is None else ctypes.byref(pc), _lib.np_ptr(psk), pocc, th_points,
                 ratio_hamming_points, projection, *[_lib.np_ptr(a) for a in p_out], None if lc is None else ctypes.byref(lc), _lib.np_ptr(lsk),
                 locc, th_lines, ratio_hamming_lines, *[_lib.np_ptr(a) for a in l_out], _lib.np_ptr(stats), stream))
    as_dict = lambda o: dict(match_idx=o[0], match_dist=o[1], reached=o[2], nmatches=o[3], stats=o[4])
    return (None if points is None else as_dict(p_out)), (None if lines is None else as_dict(l_out)), stats


# ---- SearchByBoW over resident key frames: loop detection's first stage, relocalisation
class _BowFrameC(ctypes.Structure):
    _fields_ = [("n", ctypes.c_int32), ("desc", _vp), ("angle", _vp), ("vec", _FeatVecC)]


@dataclass
class BowFrame:
    """plvs_bow_frame: what SearchByBoW(pKF, F) reads of the frame."""
    desc: np.ndarray      # F.mDescriptors, n x 32
    angle: np.ndarray     # F.mvKeys[i].angle, degrees
    vec: FeatureVector    # F.mFeatVec

    def as_c(self):
        self._d = np.ascontiguousarray(self.desc, np.uint8).reshape(-1, 32)
        self._a = np.ascontiguousarray(self.angle, np.float32)
        return _BowFrameC(self._d.shape[0], _lib.np_ptr(self._d), _lib.np_ptr(self._a), self.vec.as_c())


def _valid_list(valid, K):
    assert len(valid) == K
    keep = [None if v is None else np.ascontiguousarray(v, np.uint8) for v in valid]
    return (_vp * max(K, 1))(*[None if v is None else v.ctypes.data for v in keep]), keep


def _bow_outputs(K, n, outputs):
    """outputs: None, or (match, match_dist, nmatches, stats) to write into (the refusal tests pass their own)."""
    if outputs is not None:
        return outputs
    return np.full((K, n), -2, np.int32), np.full((K, n), -2, np.int32), np.full(K, -7, np.int32), np.full(6, -1, np.int32)


def search_by_bow_kf(kf1, valid1, key_frames2, valid2, nn_ratio=0.9, check_orientation=True, host=False, stream=None, n1=None, outputs=None):
    """ORBmatcher::SearchByBoW(pKF1, pKF2[k], vpMatches12[k]) for every k in one call (plvs_hip_orb_search_by_bow_kf / _kf_host).
    valid1 [n1], valid2[k] [n_k]: vpMapPoints[i] && !isBad().  -> dict(match_idx [K,n1], match_dist [K,n1], nmatches [K], stats [6])."""
    K = len(key_frames2)
    hs = (_vp * max(K, 1))(*[None if kf is None else kf.handle for kf in key_frames2])
    vl, keep = _valid_list(valid2, K)
    v1 = None if valid1 is None else np.ascontiguousarray(valid1, np.uint8)
    if n1 is None:
        n1 = kf1.info()["n_points"] if kf1 is not None else 0
    match_idx, match_dist, nmatches, stats = _bow_outputs(K, max(n1, 0), outputs)
    f = getattr(_lib.lib, "plvs_hip_orb_search_by_bow_kf" + ("_host" if host else ""))
    f.argtypes = [_vp, _vp, _vp, _vp, _i, _f, _i, _vp, _vp, _vp, _vp] + ([] if host else [_vp])
    args = [None if kf1 is None else kf1.handle, _lib.np_ptr(v1), hs if K else None, vl if K else None, K, nn_ratio, int(check_orientation),
            _lib.np_ptr(match_idx), _lib.np_ptr(match_dist), _lib.np_ptr(nmatches), _lib.np_ptr(stats)]
    _lib.check(f(*(args if host else args + [stream])))
    return dict(match_idx=match_idx, match_dist=match_dist, nmatches=nmatches, stats=stats)


def search_by_bow_frame_kf(key_frames, kf_valid, frame, nn_ratio=0.75, check_orientation=True, host=False, stream=None, outputs=None):
    """ORBmatcher::SearchByBoW(pKF[k], F, vvpMapPointMatches[k]) for every k in one call (plvs_hip_orb_search_by_bow_frame_kf / _kf_host).
    -> dict(assigned [K,F.n]: the key point of key frame k whose map point goes to the frame's key point, match_dist, nmatches [K], stats [6])."""
    K = len(key_frames)
    hs = (_vp * max(K, 1))(*[None if kf is None else kf.handle for kf in key_frames])
    vl, keep = _valid_list(kf_valid, K)
    fc = None if frame is None else frame.as_c()
    assigned, match_dist, nmatches, stats = _bow_outputs(K, 0 if fc is None else fc.n, outputs)
    f = getattr(_lib.lib, "plvs_hip_orb_search_by_bow_frame_kf" + ("_host" if host else ""))
    f.argtypes = [_vp, _vp, _i, _vp, _f, _i, _vp, _vp, _vp, _vp] + ([] if host else [_vp])
    args = [hs if K else None, vl if K else None, K, None if fc is None else ctypes.byref(fc), nn_ratio, int(check_orientation),
            _lib.np_ptr(assigned), _lib.np_ptr(match_dist), _lib.np_ptr(nmatches), _lib.np_ptr(stats)]
    _lib.check(f(*(args if host else args + [stream])))
    return dict(assigned=assigned, match_dist=match_dist, nmatches=nmatches, stats=stats)
