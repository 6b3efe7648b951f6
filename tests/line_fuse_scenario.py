"""Seeded scenarios for the search stage of LineMatcher::Fuse (plvs_hip_line_fuse_search).

inputs(): the set behind tests/golden/line_fuse_reference.npz — three key frames (TUM1 intrinsics, 3 line levels at 1.2, th 3) and
about 100 map lines.
  key frame 0 holds the placed key lines only, bounds -4 .. 645 x -3 .. 484 (the Frame's diagonal 811.4, the key frame's int 811).
    Its (theta, d) plane is cut into slots whose windows do not meet: five normal angles (-60, -30, 0, 30, 60 degrees) times two
    offsets d at level 0, the same angles at level 2, and two windows that wrap at -pi/2 and +pi/2.  A map line predicted at level 0
    meets key lines of octave 0 only, one predicted at level 2 those of octaves 1 and 2, so the slots carry a case each:
    a candidate; a member above the level band and one below it; a key line whose START is 5 px off the projected line (dropped by
    the start gate alone), one whose END is; one dropped by the right-image gate alone; mvuRightLineStart == 0.0f (the stereo branch:
    dropped there, where `> 0` would have accepted it); mvuRightLineEnd < 0 with a start that would fail the gate (skipped: a
    candidate); distances of exactly 60 and 61; an empty window; windows clipped at column 0 and at column 159; a window split at
    -pi/2 and one at +pi/2, each with a member on either side of the wrap whose d have opposite signs — in the second the two tie
    and the winner, in the wrapped part, has the HIGHER index.
  key frame 1: 120 random key lines, mvuRightLineStart empty.
  key frame 2: 120 random key lines with stereo, bounds 600 .. 1240 x 500 .. 980 and a principal point moved along (diagonal 800):
    lines near its far corner have d beyond the grid — their key lines are in no cell (PosLineInGrid), their windows miss the
    grid entirely.
  Most map lines are key lines of key frame 1 or 2 back-projected with a few descriptor bits flipped; the rest are the placed
  cases, among them one per rejection of ProjectLineWithCheck and of Fuse.  scripts/make_line_fuse_golden.py asserts each on the
  reference's run.  The two cases the reference leaves undefined (distMiddlePoint == 0, coinciding end points) are NOT in this set:
  degenerate_inputs() hands them to the entries alone.
random_inputs(K, M, N, seed), crowd_inputs(), ambiguous_inputs(): other sizes for the restatement and the device."""
import hashlib
import math

import numpy as np

from tests import line_fuse_restatement as R
from tests import track_local_scenario as L

f32 = np.float32
SEED = 20261021
K4, MBF = L.K4, L.MBF
N_LEVELS, SCALE_FACTORS, INV_SIGMA2, LOG_SCALE = L.N_LINE_LEVELS, L.LINE_SCALE_FACTORS, L.LINE_INV_SIGMA2, L.LOG_SCALE
BOUNDS_A = np.array([-4, 645, -3, 484], f32)
BOUNDS_B = np.array([600, 1240, 500, 980], f32)
TH = 3.0
N_KL = 120
KEYLINE_DTYPE = np.dtype([("angle", f32), ("class_id", np.int32), ("octave", np.int32), ("pt_x", f32), ("pt_y", f32), ("response", f32),
                          ("size", f32), ("startPointX", f32), ("startPointY", f32), ("endPointX", f32), ("endPointY", f32),
                          ("sPointInOctaveX", f32), ("sPointInOctaveY", f32), ("ePointInOctaveX", f32), ("ePointInOctaveY", f32),
                          ("lineLength", f32), ("numOfPixels", np.int32)])
assert KEYLINE_DTYPE.itemsize == 68        # cv::line_descriptor_c::KeyLine (include/plvs_hip.h: plvs_keyline)


def _diag(b):
    return f32(np.sqrt(f32(f32(b[1] - b[0]) ** 2 + f32(b[3] - b[2]) ** 2)))       # Frame::mnMaxDiag (src/Frame.cc:1777), a float


def _quat(axis, angle):
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    return np.concatenate([np.sin(angle / 2) * a, [np.cos(angle / 2)]])


def _rot64(q):
    x, y, z, w = (float(c) for c in q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def _poses(K):
    return [(_rot64(_quat([1.0, 2.0, 0.5 + 0.3 * k], 0.04 * k + 0.02)), np.array([0.03 * k, -0.02 * k, 0.01 * k])) for k in range(K)]


def keylines(segs, octave):
    """segs [n, 4] = startPointX, startPointY, endPointX, endPointY."""
    segs = np.asarray(segs, f32).reshape(-1, 4)
    kl = np.zeros(len(segs), KEYLINE_DTYPE)
    kl["startPointX"], kl["startPointY"], kl["endPointX"], kl["endPointY"] = segs.T
    kl["octave"] = octave
    kl["pt_x"], kl["pt_y"] = (segs[:, 0] + segs[:, 2]) / 2, (segs[:, 1] + segs[:, 3]) / 2
    kl["lineLength"] = np.hypot(segs[:, 2] - segs[:, 0], segs[:, 3] - segs[:, 1])
    kl["class_id"] = np.arange(len(segs))
    return kl


def make_kf(R64, t64, kl, desc, u_right_start, u_right_end, bounds=BOUNDS_A, offset=(0.0, 0.0)):
    Rf = np.asarray(R64, np.float64).astype(f32)
    tcw = np.asarray(t64, np.float64).astype(f32)
    K = np.array([K4[0], K4[1], K4[2] + f32(offset[0]), K4[3] + f32(offset[1])], f32)
    return dict(kl=kl, desc=np.ascontiguousarray(desc, np.uint8).reshape(-1, 32),
                u_right_start=None if u_right_start is None else np.asarray(u_right_start, f32),
                u_right_end=None if u_right_end is None else np.asarray(u_right_end, f32), mbf=float(MBF), scale_factors=SCALE_FACTORS,
                inv_level_sigma2=INV_SIGMA2, max_diag=float(_diag(bounds)), log_scale_factor=float(LOG_SCALE), K4=K,
                bounds4=np.asarray(bounds, f32), Rcw=np.ascontiguousarray(Rf.T).reshape(9), tcw=tcw,
                Ow=(-(np.asarray(R64, np.float64).T @ np.asarray(t64, np.float64))).astype(f32))


def world(kf, u, v, z):
    """The world point (f64) that projects to (u, v) at camera depth z in `kf`."""
    Rm = np.asarray(kf["Rcw"], np.float64).reshape(3, 3).T
    K = kf["K4"].astype(np.float64)
    xc = np.array([(u - K[2]) * z / K[0], (v - K[3]) * z / K[1], z])
    return Rm.T @ (xc - kf["tcw"].astype(np.float64))


def _flip(rng, d, nbits):
    d = np.array(d, np.uint8).copy()
    for b in rng.choice(256, nbits, replace=False):
        d[b // 8] ^= np.uint8(1 << (b % 8))
    return d


LEVEL_Q = {0: -0.5, 1: 0.5, 2: 1.1}      # log(ratio) / log 1.2: ceil = the level, the ratio inside the band 1 / 1.2 .. 1 / 0.8


def line_for(kf, seg, zs, ze, level, desc, q=None):
    """(start, end, normal, max_dist, desc) of a map line that projects onto `seg` in `kf` with its ends at depths zs, ze, seen
    head-on, whose predicted level there is `level`."""
    S, E = world(kf, seg[0], seg[1], zs), world(kf, seg[2], seg[3], ze)
    Mw = 0.5 * (S + E)
    PO = Mw - kf["Ow"].astype(np.float64)
    Rm = np.asarray(kf["Rcw"], np.float64).reshape(3, 3).T
    dist = np.linalg.norm(Rm @ Mw + kf["tcw"].astype(np.float64))
    return (S.astype(f32), E.astype(f32), (PO / np.linalg.norm(PO)).astype(f32), f32(dist * 1.2 ** (LEVEL_Q[level] if q is None else q)),
            np.asarray(desc, np.uint8))


def seg_at(theta_deg, cx, cy, half):
    """The segment through (cx, cy) whose normal has the angle theta, from the end with the smaller y (or x) to the other."""
    t = math.radians(theta_deg)
    dx, dy = -math.sin(t) * half, math.cos(t) * half
    return np.array([cx - dx, cy - dy, cx + dx, cy + dy], np.float64)


def _pack(lines):
    return dict(start=np.array([p[0] for p in lines], f32).reshape(-1, 3), end=np.array([p[1] for p in lines], f32).reshape(-1, 3),
                normal=np.array([p[2] for p in lines], f32).reshape(-1, 3), max_dist=np.array([p[3] for p in lines], f32),
                desc=np.array([p[4] for p in lines], np.uint8).reshape(-1, 32))


def _random_kf(rng, R64, t64, n, stereo=True, bounds=BOUNDS_A, offset=(0.0, 0.0), corner=0):
    """n random segments inside the bounds (the last `corner` of them near the far corner), random octaves and descriptors."""
    b = np.asarray(bounds, np.float64)
    cx = rng.uniform(b[0] + 50, b[1] - 50, n)
    cy = rng.uniform(b[2] + 50, b[3] - 50, n)
    if corner:
        cx[n - corner:], cy[n - corner:] = rng.uniform(b[1] - 60, b[1] - 45, corner), rng.uniform(b[3] - 60, b[3] - 45, corner)
    ang, half = rng.uniform(0, math.pi, n), rng.uniform(10, 40, n)
    if corner:
        ang[n - corner:] = rng.uniform(2.1, 2.4, corner)            # the segment's direction: its normal points at the corner
    segs = np.stack([cx - np.cos(ang) * half, cy - np.sin(ang) * half, cx + np.cos(ang) * half, cy + np.sin(ang) * half], 1)
    kl = keylines(segs, rng.integers(0, N_LEVELS, n))
    zs, ze = rng.uniform(1.0, 4.0, n), rng.uniform(1.0, 4.0, n)
    none = rng.random(n) < 0.4
    urs = np.where(none, -1.0, kl["startPointX"] - float(MBF) / zs) if stereo else None
    ure = np.where(none | (rng.random(n) < 0.1), -1.0, kl["endPointX"] - float(MBF) / ze) if stereo else None
    kf = make_kf(R64, t64, kl, rng.integers(0, 256, (n, 32), dtype=np.uint8), urs, ure, bounds, offset)
    kf["zs"], kf["ze"] = zs, ze
    return kf


def _matching_lines(rng, kfs, M, lines):
    """M map lines, each the back-projection of a random key line of one of the key frames."""
    cand = [kf for kf in kfs if len(kf["kl"]) and "zs" in kf]
    if not cand and M:       # no key frame (or none with key lines): the lines of a key frame that is not handed on
        cand = [_random_kf(rng, *_poses(1)[0], 50)]
    for i in range(M):
        kf = cand[i % len(cand)]
        j = int(rng.integers(len(kf["kl"])))
        k = kf["kl"][j]
        seg = [k["startPointX"], k["startPointY"], k["endPointX"], k["endPointY"]]
        lines.append(line_for(kf, seg, float(kf["zs"][j]), float(kf["ze"][j]), int(k["octave"]), _flip(rng, kf["desc"][j], int(rng.integers(0, 40)))))


def _public(kfs):
    return [{k: v for k, v in kf.items() if k not in ("zs", "ze")} for kf in kfs]


# the slots of key frame 0: (theta of the normal in degrees, centre) — see the head
SLOTS = {(-60, "A"): (40, 440), (-60, "B"): (600, 40), (-30, "A"): (40, 440), (-30, "B"): (600, 40), (0, "A"): (15, 240), (0, "B"): (630, 240),
         (30, "A"): (40, 40), (30, "B"): (600, 440), (60, "A"): (40, 40), (60, "B"): (600, 440)}
HALF = 25.0
Z = 2.0


def inputs():
    rng = np.random.default_rng(SEED)
    poses = _poses(3)
    kf0 = make_kf(*poses[0], keylines(np.zeros((0, 4)), 0), np.zeros((0, 32), np.uint8), np.zeros(0), np.zeros(0))
    kf1 = _random_kf(rng, *poses[1], N_KL, stereo=False)
    kf2 = _random_kf(rng, *poses[2], N_KL, stereo=True, bounds=BOUNDS_B, offset=(600.0, 500.0), corner=6)
    segs, octs, descs, urs, ure, lines, where = [], [], [], [], [], [], {}
    rd = lambda: rng.integers(0, 256, 32, dtype=np.uint8)
    disparity = float(MBF) / Z

    def kl(seg, octave, desc=None, us=-1.0, ue=-1.0):
        """us / ue: None = the consistent right-image abscissa."""
        segs.append(np.asarray(seg, np.float64))
        octs.append(octave)
        descs.append(rd() if desc is None else desc)
        urs.append(seg[0] - disparity if us is None else us)
        ure.append(seg[2] - disparity if ue is None else ue)
        return len(segs) - 1

    def line(name, p):
        where.setdefault(name, []).append(len(lines))
        lines.append(p)

    def slot(theta, which, half=HALF):
        return seg_at(theta, *SLOTS[(theta, which)], half)

    def shifted(seg, ds, de):
        """The segment with its start / end moved ds / de pixels along the normal."""
        t = math.atan2(seg[0] - seg[2], seg[3] - seg[1])            # the normal (ye - ys, xs - xe)
        n = np.array([math.cos(t), math.sin(t)])
        return np.concatenate([seg[:2] + ds * n, seg[2:] + de * n])

    s = slot(0, "A");   j = kl(s, 0);                            line("candidate_mono", line_for(kf0, s, Z, Z, 0, _flip(rng, descs[j], 5)))
    s = slot(-60, "B"); j = kl(s, 1);                            line("above_level", line_for(kf0, s, Z, Z, 0, descs[j]))
    s = slot(-30, "A"); j = kl(shifted(s, 5.0, 0.0), 0);         line("start_gate", line_for(kf0, s, Z, Z, 0, descs[j]))
    s = slot(-30, "B"); j = kl(shifted(s, 0.0, 5.0), 0);         line("end_gate", line_for(kf0, s, Z, Z, 0, descs[j]))
    s = slot(30, "A");  j = kl(s, 0, us=s[0] - disparity + 6.0, ue=s[2] - disparity + 6.0)
    line("right_gate", line_for(kf0, s, Z, Z, 0, descs[j]))
    s = slot(0, "B");   j = kl(s, 0, us=0.0, ue=None);           line("u_right_start_zero", line_for(kf0, s, Z, Z, 0, descs[j]))
    s = slot(30, "B");  j = kl(s, 0, us=5.0, ue=-1.0);           line("u_right_end_negative", line_for(kf0, s, Z, Z, 0, _flip(rng, descs[j], 4)))
    s = slot(60, "A");  j = kl(s, 0, us=None, ue=None);          line("dist_60", line_for(kf0, s, Z, Z, 0, _flip(rng, descs[j], 60)))
    s = slot(-60, "A"); j = kl(s, 0);                            line("dist_61", line_for(kf0, s, Z, Z, 0, _flip(rng, descs[j], 61)))
    line("empty_window", line_for(kf0, slot(60, "B"), Z, Z, 0, rd()))
    # level 2: the members of the level-0 slots at 30 degrees lie below its band; the two clipped windows find a key line of octave 2
    line("below_level", line_for(kf0, seg_at(30, 320, 240, HALF), Z, Z, 2, rd()))
    s = seg_at(-60, 20, 460, 15.0); j = kl(s, 2);                line("clip_column_0", line_for(kf0, s, Z, Z, 2, _flip(rng, descs[j], 3)))
    s = seg_at(0, 500, 240, HALF);  j = kl(s, 2);                line("clip_column_159", line_for(kf0, s, Z, Z, 2, _flip(rng, descs[j], 3)))
    # the window split at -pi/2: the projected line at -88 degrees, a member at -88 (d < 0) and one at +86 (d > 0, the wrapped part)
    q = rd()
    s = seg_at(-88, 320, 100, 15.0)
    j_rest = kl(s, 0, _flip(rng, q, 9))
    j_wrapped = kl(seg_at(86, 320, 100, 15.0), 0, _flip(rng, q, 6))
    line("split_minus", line_for(kf0, s, Z, Z, 0, q))
    where["split_minus_members"] = [j_wrapped, j_rest]
    # the window split at +pi/2: the projected line at +88 degrees; the member at +86 first in the array, the one at -86 (d < 0, the
    # wrapped part, listed first by GetLineFeaturesInArea) after it — both 3 bits from the line's descriptor
    q = rd()
    s = seg_at(88, 320, 460, 15.0)
    j_rest = kl(seg_at(86, 320, 460, 15.0), 0, _flip(rng, q, 3))
    j_wrapped = kl(seg_at(-86, 320, 460, 15.0), 0, _flip(rng, q, 3))
    line("split_plus_tie", line_for(kf0, s, Z, Z, 0, q))
    where["tie_indices"] = [j_wrapped, j_rest]
    # ---- key frame 2: d beyond the grid
    k2 = kf2["kl"][N_KL - 1]
    line("window_misses_grid", line_for(kf2, [k2["startPointX"], k2["startPointY"], k2["endPointX"], k2["endPointY"]], Z, Z, 0, rd()))
    # ---- the placed lines that never reach a window (key frame 0)
    mid = seg_at(10, 320, 240, HALF)
    line("middle_behind", line_for(kf0, mid, -1.5, -1.5, 1, rd()))
    line("middle_outside", line_for(kf0, seg_at(10, -60, 240, HALF), Z, Z, 1, rd()))
    line("too_near", line_for(kf0, mid, Z, Z, 1, rd(), q=1.5))         # ratio 1.2^1.5 = 1.31 > 1 / 0.8
    line("too_far", line_for(kf0, mid, Z, Z, 1, rd(), q=-1.5))         # ratio 0.76 < 1 / 1.2
    S, E = world(kf0, 300, 240, 1.0), world(kf0, 300, 240, -0.4)       # along a viewing ray through the camera: the end behind it
    p = line_for(kf0, mid, Z, Z, 1, rd())
    Rm = np.asarray(kf0["Rcw"], np.float64).reshape(3, 3).T
    dist = np.linalg.norm(Rm @ (0.5 * (S + E)) + kf0["tcw"].astype(np.float64))
    line("end_behind", (S.astype(f32), E.astype(f32), p[2], f32(dist), p[4]))
    line("end_outside", line_for(kf0, [560, 240, 690, 240], Z, Z, 1, rd()))      # the end beyond mnMaxX
    line("end_outside", line_for(kf0, [-30, 240, 40, 240], Z, Z, 1, rd()))       # the start beyond mnMinX, the middle inside
    p = list(line_for(kf0, mid, Z, Z, 1, rd())); p[2] = (-p[2]).astype(f32); line("view_angle", tuple(p))
    n_placed = len(lines)
    kf0 = make_kf(*poses[0], keylines(np.array(segs), np.array(octs)), np.array(descs, np.uint8), np.array(urs), np.array(ure))
    kfs = [kf0, kf1, kf2]
    _matching_lines(rng, kfs, 100 - n_placed - 6, lines)
    for name in ("skip_null", "skip_bad", "skip_in_kf"):
        where[name] = [len(lines), len(lines) + 1]
        _matching_lines(rng, kfs, 2, lines)
    M = len(lines)
    skip = np.zeros((3, M), np.uint8)
    for code, name in ((1, "skip_null"), (2, "skip_bad")):
        skip[:, where[name]] = code                     # for every key frame
    skip[1, where["skip_in_kf"][0]] = 3                 # in one key frame only
    skip[2, where["skip_in_kf"][1]] = 3
    return dict(kfs=_public(kfs), lines=_pack(lines), skip=skip, th=TH, where=where)


def random_inputs(K=3, M=300, N=300, seed=1, empty_kf=None):
    """K key frames of N key lines (key frame `empty_kf` of none; odd ones without stereo), M matching lines, a sprinkle of skipped
    pairs."""
    rng = np.random.default_rng(SEED + seed)
    kfs = [_random_kf(rng, Rm, t, 0 if k == empty_kf else N, stereo=(k % 2 == 0)) for k, (Rm, t) in enumerate(_poses(K))]
    lines = []
    _matching_lines(rng, kfs, M, lines)
    skip = (rng.random((K, M)) < 0.05).astype(np.uint8)
    return dict(kfs=_public(kfs), lines=_pack(lines), skip=skip, th=TH, where={})


def crowd_inputs(n=150):
    """One key frame whose `n` near-vertical key lines (octaves 1 and 2) all lie inside the window of every map line — more than two
    64-member strides.  140 of them stand left of the map lines (smaller d: earlier columns) with random descriptors, too far from
    the projected lines for the gates; the last ten stand within a pixel of them, eight carrying the map lines' descriptors a few
    bits off: every candidate, and the best match, lies beyond member 64 of the enumeration.  8 map lines at level 2."""
    rng = np.random.default_rng(SEED + 77)
    Rm, t = _poses(1)[0]
    n_near = 10
    cx = np.concatenate([rng.uniform(150, 305, n - n_near), 320.0 + rng.uniform(-0.8, 0.8, n_near)])
    ang = np.concatenate([rng.uniform(-3, 3, n - n_near), np.zeros(n_near)])
    segs = np.stack([seg_at(float(a), float(x), 240.0, 20.0) for a, x in zip(ang, cx)])
    pool = rng.integers(0, 256, (8, 32), dtype=np.uint8)
    desc = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    for i in range(8):
        desc[n - 1 - i] = _flip(rng, pool[i], 2 + i)
    order = rng.permutation(n)                              # the array order is not the grid's
    kl = keylines(segs[order], np.where(rng.random(n) < 0.7, 2, 1))
    stereo = rng.random(n) < 0.5
    kf = make_kf(Rm, t, kl, desc[order], np.where(stereo, kl["startPointX"] - float(MBF) / Z, -1.0), np.where(stereo, kl["endPointX"] - float(MBF) / Z, -1.0))
    lines = [line_for(kf, seg_at(0.0, 320.0 + dx, 240.0, 20.0), Z, Z, 2, pool[i]) for i, dx in enumerate(np.linspace(-1, 1, 8))]
    return dict(kfs=[kf], lines=_pack(lines), skip=None, th=TH, where={})


def ambiguous_inputs():
    """random_inputs(2, 65, 100) with, in key frame 0,
      lines 0 .. 11: max_dist = float(dist * 1.2^k), k = 0, 1: the quotient log(ratio) / log(1.2) lies within eps of an integer;
      lines 12 .. 23: projected normals at 45 degrees, where theta - deltaTheta (level 0: 10 degrees) meets the row edge at 35
        degrees: of 600 segments whose angle differs by steps of 5e-9 rad (the f32 world points add a noise of ~1e-6 rad), twelve
        that the restatement's rule (line_fuse_restatement.theta_rule) marks."""
    inp = random_inputs(2, 65, 100, seed=5)
    kf = inp["kfs"][0]
    ln = inp["lines"]
    fr = R.front(kf, ln)
    ok = np.flatnonzero(fr["reached"] == R.EMPTY_WINDOW)[:12]
    for n, i in enumerate(ok):
        ln["max_dist"][i] = f32(float(fr["dist"][i]) * 1.2 ** (n % 2))
    rng = np.random.default_rng(SEED + 5)
    sweep = _pack([line_for(kf, seg_at(45.0 + math.degrees(a), 320.0, 240.0, 30.0), Z, Z, 0, rng.integers(0, 256, 32, dtype=np.uint8))
                   for a in np.arange(-300, 300) * 5e-9])
    fs = R.front(kf, sweep)
    dtheta = f32(R.K_DELTA_THETA * SCALE_FACTORS[0])
    marked = []
    for i in np.flatnonzero(fs["reached"] == R.EMPTY_WINDOW):
        nx, ny, _, _ = R.representation(fs["uS"][i], fs["vS"][i], fs["uE"][i], fs["vE"][i])
        if R.theta_rule(ny, nx, dtheta)[1]:
            marked.append(int(i))
        if len(marked) == 12:
            break
    assert len(marked) == 12, "the sweep holds fewer than 12 lines with an ambiguous theta"
    free = [i for i in range(65) if i not in set(ok.tolist())][:12]
    for k in ln:
        ln[k][free] = sweep[k][marked]
    inp["skip"][0, free] = 0
    inp["where"] = dict(ambiguous_level=[int(i) for i in ok], ambiguous_theta=free)
    return inp


def degenerate_inputs():
    """The two cases the reference leaves undefined, in one key frame at the world's origin: line 0 has both end points at the
    camera centre and mfMaxDistance == 0 (every projection is a NaN, which passes the bounds; distMiddlePoint == 0 passes the band
    0 .. 0, and 0 < 0.5 * 0 does not hold), line 1 lies along the optical axis (both end points project to the principal point)."""
    inp = random_inputs(1, 4, 30, seed=8)
    kf = inp["kfs"][0]
    kf["Rcw"] = np.array([1, 0, 0, 0, 1, 0, 0, 0, 1], f32)
    kf["tcw"] = np.zeros(3, f32)
    kf["Ow"] = np.zeros(3, f32)
    ln = inp["lines"]
    ln["start"][0], ln["end"][0], ln["max_dist"][0] = (0.0, 0.0, 0.0), (0.0, 0.0, 0.0), 0.0
    ln["start"][1], ln["end"][1] = (0.0, 0.0, 1.0), (0.0, 0.0, 3.0)
    ln["normal"][1], ln["max_dist"][1] = (0.0, 0.0, 1.0), 2.0
    inp["skip"] = None
    return inp


def digest(inp):
    h = hashlib.sha1()
    for kf in inp["kfs"]:
        for k in ("kl", "desc", "u_right_start", "u_right_end", "scale_factors", "inv_level_sigma2", "K4", "bounds4", "Rcw", "tcw", "Ow"):
            if kf[k] is not None:
                h.update(np.ascontiguousarray(kf[k]).tobytes())
        h.update(np.array([kf["max_diag"], kf["log_scale_factor"], kf["mbf"]], f32).tobytes())
    for k in ("start", "end", "normal", "max_dist", "desc"):
        h.update(np.ascontiguousarray(inp["lines"][k]).tobytes())
    if inp["skip"] is not None:
        h.update(np.ascontiguousarray(inp["skip"]).tobytes())
    h.update(np.array([inp["th"]], f32).tobytes())
    return h.hexdigest()


def views(inp):
    """-> (list of linematcher.LineFuseKeyFrame, linematcher.FuseLines)."""
    from plvs_amd.linematcher import FuseLines, LineFuseKeyFrame, line_frame_view
    kfs = [LineFuseKeyFrame(line_frame_view(kf["kl"], kf["desc"], kf["scale_factors"], kf["inv_level_sigma2"], kf["max_diag"], kf["u_right_start"],
                                            kf["u_right_end"], kf["mbf"]), kf["log_scale_factor"], kf["K4"], kf["bounds4"], kf["Rcw"],
                            kf["tcw"], kf["Ow"]) for kf in inp["kfs"]]
    p = inp["lines"]
    return kfs, FuseLines(p["start"], p["end"], p["normal"], p["max_dist"], p["desc"])
