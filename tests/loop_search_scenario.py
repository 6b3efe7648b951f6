"""Seeded scenarios for the loop-closing SearchByProjection searches (plvs_hip_orb_loop_search_by_projection_kf,
plvs_hip_line_loop_search_by_projection_kf, the combined entry and the host twins).

point_inputs(): the set behind tests/golden/loop_search_reference.npz.  It is tests/loop_fuse_scenario.point_inputs() — three key
frames under Sim3 poses with a placed case for every reached code, the tie whose winner is not the lowest index, the zero depths, the
clipped windows — followed by what only a greedy search tells apart, placed in the rows y = 370 and y = 440 of key frame 0 that
nothing else uses (where[...]; scripts/make_loop_search_golden.py asserts each on the reference's run):
  second_best        two points over the same two key points A, B, both nearest A: the first takes A, the second finds A claimed and
                     takes B;
  all_claimed        two points over ONE key point: the second finds every banded member claimed, bestDist stays 256;
  at_50 .. at_76     a lone key point at descriptor distance 50, 51, 75, 76: TH_LOW * 1.0 = 50 and TH_LOW * 1.5 = 75 on both sides;
  occupied_wins      two key points, the nearer one marked in `occupied` (vpMatched not null on entry): the point takes the other;
  project_bit        a point whose u differs in the last bit between Pinhole::project and the invz projection, over a lone key point
                     placed at the edge of its window so that fabs(kx - u) < radius holds for one u and not for the other.
RUNS: the two (projection, ratio) pairs the golden holds, th = 4 as the set was placed.
line_inputs(): tests/loop_fuse_scenario.line_inputs() — three key frames, every rejection of ProjectLineWithCheck and of the search, the
windows split at -pi/2 and +pi/2 with the tie won in the wrapped part — plus a FOURTH key frame that holds the greedy cases alone.  A
line's window is +-10 degrees (level 0) by +-th * 100 px: the cases sit 25 degrees apart around the image centre, seven at level 0
(key lines of octave 0):
  second_best (-75 degrees), all_claimed (-50), at_60 (-25), at_61 (0), at_90 (25), at_91 (50: TH_LOW * 1.0 = 60, * 1.5 = 90),
  occupied_wins (75).
LINE_RUNS: (overload, ratio) — the two line overloads share one search, the overload tells only which vectors are written.
crowd_line_inputs(): tests/loop_fuse_scenario.crowd_line_inputs()'s key frame and lines plus a second key frame of LIST_LEN + 2 key lines
of ONE descriptor on one segment, and LIST_LEN + 2 lines landing on them.
crowd_point_inputs(): tests/orb_fuse_scenario.crowd_inputs() (a window over 200 key points from a pool of four descriptors) plus
LIST_LEN + 2 key points of ONE descriptor in one cell and LIST_LEN + 2 points landing on them: the posted list is truncated and
wholly claimed for the last two, which the host evaluates again.
random_point_inputs: other sizes for the restatement and the device."""
import hashlib

import numpy as np

from tests import line_fuse_scenario as LS
from tests import loop_fuse_scenario as LF
from tests import loop_search_restatement as R
from tests import orb_fuse_scenario as PS

f32 = np.float32
TH = LF.TH
SEED = 20261101
RUNS = (("camera_r15", R.CAMERA, 1.5), ("invz_r10", R.INVZ, 1.0))
LINE_RUNS = (("kf0_r15", 0, 1.5), ("kf1_r10", 1, 1.0))
LIST_LEN = R.LIST_LEN
LVL = 4


def _append_kps(kf, xs, ys, octaves, descs):
    n0 = len(kf["x"])
    kf["x"] = np.concatenate([kf["x"], np.asarray(xs, f32)])
    kf["y"] = np.concatenate([kf["y"], np.asarray(ys, f32)])
    kf["octave"] = np.concatenate([kf["octave"], np.asarray(octaves, np.int32)])
    kf["u_right"] = np.concatenate([kf["u_right"], np.full(len(xs), -1, f32)])
    kf["desc"] = np.concatenate([kf["desc"], np.asarray(descs, np.uint8).reshape(-1, 32)])
    return list(range(n0, n0 + len(xs)))


def _project_bit_case(kf0, y, rng):
    """-> (point tuple, key point x, y): see the head.  Searched over sub-pixel positions right of x = 180."""
    sf = np.asarray(kf0["scale_factors"], f32)
    radius = f32(TH) * sf[LVL]
    for step in range(4000):
        p = PS._point_for(kf0, 180.0 + 0.013 * step, y, 2.0, LVL, rng.integers(0, 256, 32, dtype=np.uint8))
        one = dict(pos=p[0].reshape(1, 3), normal=p[1].reshape(1, 3), min_dist=np.array([p[2]], f32), max_dist=np.array([p[3]], f32))
        cam, inv = R.front(kf0, one, R.CAMERA), R.front(kf0, one, R.INVZ)
        if cam["u"][0] == inv["u"][0] or cam["reached"][0] != R.PR.EMPTY_WINDOW or inv["reached"][0] != R.PR.EMPTY_WINDOW:
            continue
        lo, hi = sorted((f32(cam["u"][0]), f32(inv["u"][0])))
        kx = f32(lo + radius)
        for _ in range(64):          # the smallest kx with kx - lo >= radius
            if f32(np.nextafter(kx, f32(-np.inf))) - lo >= radius:
                kx = f32(np.nextafter(kx, f32(-np.inf)))
            elif kx - lo < radius:
                kx = f32(np.nextafter(kx, f32(np.inf)))
            else:
                break
        if abs(f32(kx - hi)) < radius and not abs(f32(kx - lo)) < radius:
            return p, kx, f32(np.asarray(cam["v"])[0])
    raise AssertionError("no point whose two projections differ in the last bit of u")


def point_inputs():
    base = LF.point_inputs()
    rng = np.random.default_rng(SEED)
    kfs = [dict(kf) for kf in base["kfs"]]
    kf0, where = kfs[0], dict(base["where"])
    pts, new = base["points"], []
    M0 = len(pts["min_dist"])
    rd = lambda: rng.integers(0, 256, 32, dtype=np.uint8)

    def point(name, u, v, desc):
        where.setdefault(name, []).append(M0 + len(new))
        new.append(PS._point_for(kf0, u, v, 2.0, LVL, desc))

    # second_best: A at 260, B at 263
    dA = rd()
    dB = PS._flip(rng, dA, 10)
    where["second_best_members"] = _append_kps(kf0, [260, 263], [370, 370], [LVL, LVL], [dA, dB])
    point("second_best_first", 261, 370, PS._flip(rng, dA, 2))
    point("second_best", 262, 370, PS._flip(rng, dA, 3))
    # all_claimed: C at 320
    dC = rd()
    where["all_claimed_member"] = _append_kps(kf0, [320], [370], [LVL], [dC])
    point("all_claimed_first", 320, 370, PS._flip(rng, dC, 2))
    point("all_claimed", 321, 370, PS._flip(rng, dC, 4))
    # a lone key point at each distance around both thresholds
    for x, bits in ((380, 50), (440, 51), (500, 75), (560, 76)):
        d = rd()
        _append_kps(kf0, [x], [370], [LVL], [d])
        point(f"at_{bits}", x, 370, PS._flip(rng, d, bits))
    # occupied_wins: E at 60 (occupied on entry), F at 63
    dE = rd()
    dF = PS._flip(rng, dE, 12)
    where["occupied_members"] = _append_kps(kf0, [60, 63], [440, 440], [LVL, LVL], [dE, dF])
    point("occupied_wins", 61, 440, PS._flip(rng, dE, 2))
    # project_bit
    p, kx, ky = _project_bit_case(kf0, 440.0, rng)
    where["project_bit_member"] = _append_kps(kf0, [kx], [ky], [LVL], [PS._flip(rng, p[4], 3)])
    where["project_bit"] = [M0 + len(new)]
    new.append(p)
    add = PS._pack(new)
    points = {k: np.concatenate([pts[k], add[k]]) for k in pts}
    skip = np.concatenate([base["skip"], np.zeros((3, len(new)), np.uint8)], 1)
    occupied = [np.zeros(len(kf["x"]), np.uint8) for kf in kfs]
    occupied[0][where["occupied_members"][0]] = 1
    occupied[1] = None                                  # a NULL entry among the others
    return dict(kfs=kfs, points=points, skip=skip, occupied=occupied, th=TH, where=where)


def crowd_point_inputs():
    base = LF.crowd_point_inputs()
    rng = np.random.default_rng(SEED + 1)
    kf = dict(base["kfs"][0])
    lvl = PS.N_LEVELS - 1
    d = rng.integers(0, 256, 32, dtype=np.uint8)
    n = LIST_LEN + 2
    # one cell (10 px wide) far from the crowd at (322, 241): x in 500.5 .. 503, y = 100
    members = _append_kps(kf, 500.5 + 0.5 * np.arange(n), np.full(n, 100.0), np.full(n, lvl), np.tile(d, (n, 1)))
    new = [PS._point_for(kf, 501.0 + 0.2 * i, 100.0, 2.0, lvl, PS._flip(rng, d, i)) for i in range(n)]
    add = PS._pack(new)
    M0 = len(base["points"]["min_dist"])
    points = {k: np.concatenate([base["points"][k], add[k]]) for k in base["points"]}
    where = dict(same_descriptor_members=members, same_descriptor_points=list(range(M0, M0 + n)))
    return dict(kfs=[kf], points=points, skip=None, occupied=None, th=TH, where=where)


def random_point_inputs(K=3, M=300, N=300, seed=1, empty_kf=None, occupied_fraction=0.1):
    """tests/loop_fuse_scenario.random_point_inputs with `occupied`: a fraction of every key frame's key points, key frame 1's NULL."""
    base = LF.random_point_inputs(K, M, N, seed, empty_kf)
    rng = np.random.default_rng(SEED + 7 + seed)
    occupied = [(rng.random(len(kf["x"])) < occupied_fraction).astype(np.uint8) for kf in base["kfs"]]
    if K > 1:
        occupied[1] = None
    return dict(base, occupied=occupied)


def repeated_point_inputs(K, M, N=200, seed=3):
    """K key frames that are ONE key frame under K poses a little apart (the verification loop's shape: the same matched key frame's
    points searched under the poses of the current key frame's covisibles), M points."""
    base = LF.random_point_inputs(1, M, N, seed)
    kf = base["kfs"][0]
    kfs = []
    for k in range(K):
        c = dict(kf, tcw=(np.asarray(kf["tcw"], f32) + f32(0.002 * k)).astype(f32))
        c["Ow"] = (-(PS._rot64(c["q_cw"]).T @ c["tcw"].astype(np.float64))).astype(f32)
        kfs.append(LF.sim3_of(c, LF.SCALES[k % 3]))
    skip = np.tile(base["skip"], (K, 1)) if K else np.zeros((0, M), np.uint8)
    return dict(kfs=kfs, points=base["points"], skip=skip, occupied=None, th=TH, where={})


def nominal_point_inputs(K=5, M=5000, N=1500, seed=11):
    """The measurement's shape (scripts/measure_loop_search.py): the verification loop of src/LoopClosing.cc:1021-1044 — K covisible
    key frames a few centimetres and degrees apart, N key points each, and the matched key frame's M map points, each the
    back-projection of a key point of one of them; th = 3, ratio 1.5 as :1237 calls it."""
    rng = np.random.default_rng(SEED + seed)
    kfs = [PS._random_kf(rng, q, t, N, PS.H - 12.0) for q, t in PS._poses(K)]
    pts = []
    PS._matching_points(rng, kfs, M, pts)
    skip = (rng.random((K, M)) < 0.02).astype(np.uint8) * 2
    return dict(kfs=LF._as("points", PS._public(kfs), LF.SCALES), points=PS._pack(pts), skip=skip, occupied=None, th=3.0, where={})


def _line_kf(k, segs, octaves, descs, scale):
    """A key frame of the given key lines alone (no right image) under pose k of the line scenario and a Sim3 scale."""
    kf = LS.make_kf(*LS._poses(k + 1)[k], LS.keylines(np.asarray(segs, np.float64).reshape(-1, 4), np.asarray(octaves, np.int32)),
                    np.asarray(descs, np.uint8).reshape(-1, 32), None, None)
    c = LF.sim3_of(kf, scale)
    c["Ow"] = c["Ow_lines"]
    return c


def line_inputs():
    base = LF.line_inputs()
    rng = np.random.default_rng(SEED + 2)
    rd = lambda: rng.integers(0, 256, 32, dtype=np.uint8)
    segs, descs, new, where = [], [], [], dict(base["where"])
    M0 = len(base["lines"]["max_dist"])
    seg = lambda theta, shift=0.0: LF._shifted(LS.seg_at(theta, 320, 240, LS.HALF), shift, shift)

    def kl(s, d):
        segs.append(s)
        descs.append(d)
        return len(segs) - 1

    cases = []          # (name, segment the line projects onto, descriptor): the lines need the key frame, built below

    def line(name, s, d):
        where.setdefault(name, []).append(M0 + len(cases))
        cases.append((s, d))

    dA = rd()
    where["second_best_members"] = [kl(seg(-75), dA), kl(seg(-75, 2.0), LS._flip(rng, dA, 10))]
    line("second_best_first", seg(-75, 0.5), LS._flip(rng, dA, 2))
    line("second_best", seg(-75, 1.0), LS._flip(rng, dA, 3))
    dC = rd()
    where["all_claimed_member"] = [kl(seg(-50), dC)]
    line("all_claimed_first", seg(-50), LS._flip(rng, dC, 2))
    line("all_claimed", seg(-50, 1.0), LS._flip(rng, dC, 4))
    for theta, bits in ((-25, 60), (0, 61), (25, 90), (50, 91)):
        d = rd()
        kl(seg(theta), d)
        line(f"at_{bits}", seg(theta), LS._flip(rng, d, bits))
    dE = rd()
    where["occupied_members"] = [kl(seg(75), dE), kl(seg(75, 2.0), LS._flip(rng, dE, 12))]
    line("occupied_wins", seg(75, 0.5), LS._flip(rng, dE, 2))
    kf3 = _line_kf(3, segs, np.zeros(len(segs), np.int32), descs, 1.7)
    add = LS._pack([LS.line_for(kf3, s, LS.Z, LS.Z, 0, d) for s, d in cases])
    lines = {k: np.concatenate([base["lines"][k], add[k]]) for k in base["lines"]}
    kfs = [dict(kf) for kf in base["kfs"]] + [kf3]
    skip = np.zeros((4, M0 + len(cases)), np.uint8)
    skip[:3, :M0] = base["skip"]
    skip[3, :M0] = base["skip"][0]
    occupied = [np.zeros(len(kf["kl"]), np.uint8) for kf in kfs]
    occupied[3][where["occupied_members"][0]] = 1
    occupied[1] = None
    return dict(kfs=kfs, lines=lines, skip=skip, occupied=occupied, th=TH, where=where)


def crowd_line_inputs():
    base = LF.crowd_line_inputs()
    rng = np.random.default_rng(SEED + 3)
    d = rng.integers(0, 256, 32, dtype=np.uint8)
    n = LIST_LEN + 2
    s = LS.seg_at(20, 320, 240, LS.HALF)
    kf1 = _line_kf(1, [LF._shifted(s, 0.3 * j, 0.3 * j) for j in range(n)], np.zeros(n, np.int32), np.tile(d, (n, 1)), 0.6)
    add = LS._pack([LS.line_for(kf1, LF._shifted(s, 0.1 * i, 0.1 * i), LS.Z, LS.Z, 0, LS._flip(rng, d, i)) for i in range(n)])
    M0 = len(base["lines"]["max_dist"])
    lines = {k: np.concatenate([base["lines"][k], add[k]]) for k in base["lines"]}
    where = dict(same_descriptor_members=list(range(n)), same_descriptor_lines=list(range(M0, M0 + n)))
    return dict(kfs=[dict(base["kfs"][0]), kf1], lines=lines, skip=None, occupied=None, th=TH, where=where)


def random_line_inputs(K=3, M=300, N=300, seed=1, empty_kf=None, occupied_fraction=0.1):
    base = LF.random_line_inputs(K, M, N, seed, empty_kf)
    rng = np.random.default_rng(SEED + 9 + seed)
    occupied = [(rng.random(len(kf["kl"])) < occupied_fraction).astype(np.uint8) for kf in base["kfs"]]
    if K > 1:
        occupied[1] = None
    return dict(base, occupied=occupied)


def nominal_line_inputs(K=5, M=1000, N=300, seed=11):
    """The line half of nominal_point_inputs: K key frames of N key lines, M map lines, th = 3."""
    rng = np.random.default_rng(SEED + 50 + seed)
    kfs = [LS._random_kf(rng, Rm, t, N, stereo=False) for Rm, t in LS._poses(K)]
    lines = []
    LS._matching_lines(rng, kfs, M, lines)
    skip = (rng.random((K, M)) < 0.02).astype(np.uint8) * 2
    return dict(kfs=LF._as("lines", LS._public(kfs), LF.SCALES), lines=LS._pack(lines), skip=skip, occupied=None, th=3.0, where={})


def digest(inp):
    h = hashlib.sha1(LF.digest(inp).encode())
    for o in inp["occupied"] or []:
        h.update(b"null" if o is None else np.ascontiguousarray(o, np.uint8).tobytes())
    return h.hexdigest()


Handles = LF.Handles
