"""Seeded scenarios for the Sim3 Fuse searches of LoopClosing::SearchAndFuse (plvs_hip_orb_loop_fuse_search_kf,
plvs_hip_line_loop_fuse_search_kf), th = 4 as src/LoopClosing.cc calls them.

point_inputs() / line_inputs(): the sets behind tests/golden/loop_fuse_reference.npz.  They are the sets of tests/orb_fuse_scenario.py
and tests/line_fuse_scenario.py — three key frames each, with their placed cases for every reached code, the tie whose winner is not
the lowest index, the pair above TH_LOW, z == +0.0f with a NaN and with an infinite projection, the windows clipped at every edge,
the windows split at -pi/2 and +pi/2 — under Sim3 poses of scales 1.7, 0.6 and 4 (sim3_of), plus what only the Sim3 overloads tell
apart (where[...]; scripts/make_loop_fuse_golden.py asserts each on the reference's run, and on the SE3 restatement the opposite):
  points  chi2_far         the window's only member 3.8 * scale px off the projection: e2 * invSigma2 = 14.4, far outside the SE3
                           overload's 5.99, inside the level band — Sim3 takes it, SE3 drops it;
          chi2_stereo_far  the same with mvuRight 30 px off (the SE3 overload's 7.8);
          (and the SE3 scenario's mono_gate, stereo_gate and u_right_zero members, which are candidates here)
  lines   sigma_level      a line predicted at level 2 over a key line of octave 1 whose ends lie 2.6 px off the projected line:
                           6.76 * invSigma2[2] = 3.26 <= 3.84 < 4.69 = 6.76 * invSigma2[1] — taken with [nPredictedLevel], dropped
                           with [klLevel];
          right_far        a key line on the projected line whose right-image abscissae are 40 px off: the SE3 overload's
                           right-image gate drops it, the Sim3 overload has none.
skip: 2 = isBad(), 3 = in the snapshot spAlreadyFound (the Sim3 overloads dereference every pointer: no null entries).
A scale that is a power of two leaves tcw = Scw.translation() / scale what the SE3 scenario had, bit for bit: key frame 2 of the
points (the zero depths need its exact translation) and the ambiguous sets use such scales.
random_*_inputs, crowd_*_inputs, ambiguous_*_inputs: other sizes for the restatement and the device."""
import hashlib

import numpy as np

from tests import line_fuse_scenario as LS
from tests import orb_fuse_scenario as PS

f32 = np.float32
TH = 4.0
SCALES = (1.7, 0.6, 4.0)
SEED = 20261022


def sim3_of(kf, scale):
    """The key frame under Scw = (scale, R, scale * tcw): the fields of plvs_keyframe_sim3_pose, with scale and s_t =
    Scw.translation() for the maker's compiled run.  tcw is the f32 quotient s_t / scale; Ow_points is the SE3 scenario's camera
    centre (an f64 evaluation, rounded); Ow_lines is -Rcw.transpose() * tcw as the f32 expression evaluates:
    (-R(0, i)) * t0 + ((-R(1, i)) * t1 + (-R(2, i)) * t2)."""
    s = f32(scale)
    if "q_cw" in kf and kf["q_cw"] is not None:
        q = np.asarray(kf["q_cw"], f32)
        Rm = PS._rot64(q).astype(f32)
    else:
        q = np.zeros(4, f32)
        Rm = np.asarray(kf["Rcw"], f32).reshape(3, 3).T
    s_t = (np.asarray(kf["tcw"], np.float64) * float(s)).astype(f32)
    tcw = (s_t / s).astype(f32)
    ow_l = np.array([f32(f32(-Rm[0, i]) * tcw[0]) + f32(f32(f32(-Rm[1, i]) * tcw[1]) + f32(f32(-Rm[2, i]) * tcw[2])) for i in range(3)], f32)
    out = dict(kf, q_cw=q, Rcw=np.ascontiguousarray(Rm.T).reshape(9), tcw=tcw, scale=float(s), s_t=s_t, Ow_points=np.asarray(kf["Ow"], f32).copy(),
               Ow_lines=ow_l)
    return out


def _as(kind, kfs, scales):
    ow = "Ow_points" if kind == "points" else "Ow_lines"
    out = []
    for k, kf in enumerate(kfs):
        c = sim3_of(kf, scales[k % len(scales)])
        c["Ow"] = c[ow]          # what the SE3 scenario's helpers (world, _point_for, line_for) and restatements read
        out.append(c)
    return out


def _skip(skip):
    return None if skip is None else np.where(skip == 1, 2, skip).astype(np.uint8)


def point_inputs():
    base = PS.inputs()
    rng = np.random.default_rng(SEED)
    kfs = _as("points", base["kfs"], SCALES)
    kf0, where = kfs[0], dict(base["where"])
    lvl = 4
    sf = float(PS.SCALE_FACTORS[lvl])
    n0 = len(kf0["x"])
    d_a, d_b = rng.integers(0, 256, 32, dtype=np.uint8), rng.integers(0, 256, 32, dtype=np.uint8)
    kf0["x"] = np.concatenate([kf0["x"], np.array([60 + 3.8 * sf, 180 + 0.5], f32)])
    kf0["y"] = np.concatenate([kf0["y"], np.array([370, 370], f32)])
    kf0["octave"] = np.concatenate([kf0["octave"], np.array([lvl, lvl - 1], np.int32)])
    kf0["u_right"] = np.concatenate([kf0["u_right"], np.array([-1, 180.5 - float(PS.MBF) / 2.0 + 30.0], f32)])
    kf0["desc"] = np.concatenate([kf0["desc"], np.stack([d_a, d_b])])
    new = [PS._point_for(kf0, 60, 370, 2.0, lvl, PS._flip(rng, d_a, 3)), PS._point_for(kf0, 180, 370, 2.0, lvl, PS._flip(rng, d_b, 3))]
    pts = base["points"]
    M = len(pts["min_dist"])
    add = PS._pack(new)
    points = {k: np.concatenate([pts[k], add[k]]) for k in pts}
    where["chi2_far"], where["chi2_stereo_far"] = [M], [M + 1]
    where["chi2_members"] = [n0, n0 + 1]
    skip = np.concatenate([_skip(base["skip"]), np.zeros((3, 2), np.uint8)], 1)
    return dict(kfs=kfs, points=points, skip=skip, th=TH, where=where)


def _shifted(seg, ds, de):
    """The segment with its start / end moved ds / de pixels along its normal."""
    t = np.arctan2(seg[0] - seg[2], seg[3] - seg[1])
    n = np.array([np.cos(t), np.sin(t)])
    return np.concatenate([seg[:2] + ds * n, seg[2:] + de * n])


def line_inputs():
    base = LS.inputs()
    rng = np.random.default_rng(SEED + 1)
    kfs = _as("lines", base["kfs"], SCALES)
    kf0, where = kfs[0], dict(base["where"])
    n0 = len(kf0["kl"])
    disparity = float(LS.MBF) / LS.Z
    s_sig, s_right = LS.seg_at(45, 320, 240, LS.HALF), LS.seg_at(-45, 320, 240, LS.HALF)
    d_a, d_b = rng.integers(0, 256, 32, dtype=np.uint8), rng.integers(0, 256, 32, dtype=np.uint8)
    kf0["kl"] = np.concatenate([kf0["kl"], LS.keylines(np.stack([_shifted(s_sig, 2.6, 2.6), s_right]), np.array([1, 0]))])
    kf0["kl"]["class_id"] = np.arange(len(kf0["kl"]))
    kf0["desc"] = np.concatenate([kf0["desc"], np.stack([d_a, d_b])])
    kf0["u_right_start"] = np.concatenate([kf0["u_right_start"], np.array([-1, s_right[0] - disparity + 40.0], f32)])
    kf0["u_right_end"] = np.concatenate([kf0["u_right_end"], np.array([-1, s_right[2] - disparity + 40.0], f32)])
    new = [LS.line_for(kf0, s_sig, LS.Z, LS.Z, 2, LS._flip(rng, d_a, 3)), LS.line_for(kf0, s_right, LS.Z, LS.Z, 0, LS._flip(rng, d_b, 4))]
    lines = base["lines"]
    M = len(lines["max_dist"])
    add = LS._pack(new)
    lines = {k: np.concatenate([lines[k], add[k]]) for k in lines}
    where["sigma_level"], where["right_far"] = [M], [M + 1]
    where["sim3_members"] = [n0, n0 + 1]
    skip = np.concatenate([_skip(base["skip"]), np.zeros((3, 2), np.uint8)], 1)
    return dict(kfs=kfs, lines=lines, skip=skip, th=TH, where=where)


def random_point_inputs(K=3, M=300, N=300, seed=1, empty_kf=None):
    base = PS.random_inputs(K, M, N, seed, empty_kf)
    return dict(base, kfs=_as("points", base["kfs"], SCALES), skip=_skip(base["skip"]), th=TH)


def random_line_inputs(K=3, M=300, N=300, seed=1, empty_kf=None):
    base = LS.random_inputs(K, M, N, seed, empty_kf)
    return dict(base, kfs=_as("lines", base["kfs"], SCALES), skip=_skip(base["skip"]), th=TH)


def crowd_point_inputs():
    base = PS.crowd_inputs()
    return dict(base, kfs=_as("points", base["kfs"], (0.6,)), th=TH)


def crowd_line_inputs():
    base = LS.crowd_inputs()
    return dict(base, kfs=_as("lines", base["kfs"], (1.7,)), th=TH)


def ambiguous_point_inputs():
    """tests/orb_fuse_scenario.ambiguous_inputs() under scales 2 and 0.5: the same translations, the same quotients within eps of an
    integer."""
    base = PS.ambiguous_inputs()
    return dict(base, kfs=_as("points", base["kfs"], (2.0, 0.5)), skip=_skip(base["skip"]), th=TH)


def ambiguous_line_inputs():
    """tests/line_fuse_scenario.ambiguous_inputs() under scales 2 and 0.5 (the distance and theta depend on Rcw and tcw alone), searched
    with ITS th: theta's ambiguity was searched for at that window."""
    base = LS.ambiguous_inputs()
    return dict(base, kfs=_as("lines", base["kfs"], (2.0, 0.5)), skip=_skip(base["skip"]))


def _ring_pose(k, K):
    """Key frame k of K looking outwards from a ring: a yaw of 360 / K degrees per key frame, so that a point one key frame sees
    lies in the image of the few key frames next to it and behind or beside all the others."""
    yaw = 2.0 * np.pi * k / K
    return PS._quat([0.05, 1.0, 0.02], yaw), np.array([0.02 * np.cos(yaw), -0.01, 0.02 * np.sin(yaw)], f32)


def nominal_point_inputs(K=30, M=10000, N=1500, seed=9):
    """The measurement's loop shape (scripts/measure_loop_fuse.py): K key frames on a ring of N key points each, M loop points, each
    the back-projection of a key point of one key frame; a minority of the K x M pairs survives the projection's tests."""
    rng = np.random.default_rng(SEED + seed)
    kfs = [PS._random_kf(rng, *_ring_pose(k, K), N, PS.H - 12.0) for k in range(K)]
    pts = []
    PS._matching_points(rng, kfs, M, pts)
    skip = (rng.random((K, M)) < 0.02).astype(np.uint8) * 2
    return dict(kfs=_as("points", PS._public(kfs), SCALES), points=PS._pack(pts), skip=skip, th=TH, where={})


def nominal_line_inputs(K=30, M=2000, N=300, seed=9):
    rng = np.random.default_rng(SEED + 100 + seed)
    kfs = []
    for k in range(K):
        q, t = _ring_pose(k, K)
        kfs.append(LS._random_kf(rng, PS._rot64(q), t.astype(np.float64), N, stereo=(k % 2 == 0)))
    lines = []
    LS._matching_lines(rng, kfs, M, lines)
    skip = (rng.random((K, M)) < 0.02).astype(np.uint8) * 2
    return dict(kfs=_as("lines", LS._public(kfs), SCALES), lines=LS._pack(lines), skip=skip, th=TH, where={})


def digest(inp):
    kind = "points" if "points" in inp else "lines"
    h = hashlib.sha1((PS if kind == "points" else LS).digest(dict(inp, kfs=[dict(kf) for kf in inp["kfs"]])).encode())
    for kf in inp["kfs"]:
        for k in ("q_cw", "Rcw", "tcw", "s_t", "Ow_points", "Ow_lines"):
            h.update(np.ascontiguousarray(kf[k], f32).tobytes())
        h.update(np.array([kf["scale"]], f32).tobytes())
    return h.hexdigest()


def poses(kfs):
    """-> list of plvs_amd.keyframe.Sim3Pose."""
    from plvs_amd.keyframe import Sim3Pose
    return [Sim3Pose(kf["q_cw"], kf["Rcw"], kf["tcw"], kf["Ow_points"], kf["Ow_lines"]) for kf in kfs]


class Handles:
    """Resident handles of a point and / or a line set (one key-frame list for both kinds), their Sim3 poses, closed on exit.  With
    both kinds the pose is the line set's with the point set's quaternion."""

    def __init__(self, points_inp=None, lines_inp=None, host_only=False):
        from plvs_amd.keyframe import ResidentKeyFrame, Sim3Pose
        pk = lk = self.points = self.lines = None
        if points_inp is not None:
            pk, self.points = PS.views(points_inp)
        if lines_inp is not None:
            lk, self.lines = LS.views(lines_inp)
        src = lines_inp if lines_inp is not None else points_inp
        self.poses = poses(src["kfs"])
        if points_inp is not None and lines_inp is not None:
            assert len(pk) == len(lk)
            self.poses = [Sim3Pose(p["q_cw"], l["Rcw"], l["tcw"], l["Ow_points"], l["Ow_lines"]) for p, l in zip(points_inp["kfs"], lines_inp["kfs"])]
        K = len(src["kfs"])
        self.kfs = [ResidentKeyFrame(None if pk is None else pk[k], None if lk is None else lk[k], host_only=host_only) for k in range(K)]

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        for kf in self.kfs:
            kf.close()
