"""Seeded scenarios for the search stage of ORBmatcher::Fuse (plvs_hip_orb_fuse_search).

inputs(): the set behind tests/golden/orb_fuse_reference.npz — three 640 x 480 key frames (TUM1 intrinsics, 8 levels at 1.2) of 200
key points each, poses a few centimetres and degrees apart, and about 100 map points.  Most points are key points of one of the
key frames back-projected at a depth with a few descriptor bits flipped, their mfMaxDistance chosen so that the predicted level is
the key point's octave: they are candidates in their own key frame and meet whatever lies at their projection in the other two.
The rest are placed cases in key frame 0, listed in inputs()["where"], whose key points sit alone in the band 320 <= y < 450 that
the random key points leave free; scripts/make_orb_fuse_golden.py asserts each on the reference's run:
  skipped (null / bad / already in the key frame), behind, outside the image, z == +0.0f with a NaN and with an infinite projection,
  too near, too far, a grazing normal, the camera centre of key frame 1 as a map point, an empty window, a window whose only
  member lies one level below the band / one above / outside the mono gate / outside the stereo gate, a key point with
  mvuRight == 0.0f (the stereo branch: dropped by er, where `> 0` would have accepted it), a best distance above TH_LOW, windows
  clipped at each grid edge, and a tie of two equal distances whose first member in enumeration order has the HIGHER index.
random_inputs(K, M, N, seed), crowd_inputs(), ambiguous_inputs(): other sizes for the restatement and the device.
replay_inputs(): a small map for the replay of INTEGRATION.md (tests/orb_fuse_replay.py)."""
import hashlib

import numpy as np

from tests import orb_fuse_restatement as R
from tests import track_local_scenario as L

f32 = np.float32
SEED = 20261020
W, H, K4, MBF, BOUNDS4 = L.W, L.H, L.K4, L.MBF, L.BOUNDS4
N_LEVELS, SCALE_FACTORS, LOG_SCALE = L.N_LEVELS, L.SCALE_FACTORS, L.LOG_SCALE
INV_SIGMA2 = (f32(1.0) / (SCALE_FACTORS * SCALE_FACTORS)).astype(f32)
GRID_W_INV, GRID_H_INV = L.GRID_W_INV, L.GRID_H_INV
TH = 3.0
N_KP = 200


def _quat(axis, angle):
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    return np.concatenate([np.sin(angle / 2) * a, [np.cos(angle / 2)]]).astype(f32)


def _rot64(q):
    x, y, z, w = (float(c) for c in q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def make_kf(q, tcw, x, y, octave, u_right, desc, Ow=None):
    q, tcw = np.asarray(q, f32), np.asarray(tcw, f32)
    if Ow is None:
        Ow = (-(_rot64(q).T @ tcw.astype(np.float64))).astype(f32)
    return dict(x=np.asarray(x, f32), y=np.asarray(y, f32), octave=np.asarray(octave, np.int32), u_right=np.asarray(u_right, f32),
                desc=np.ascontiguousarray(desc, np.uint8).reshape(-1, 32), min_x=float(BOUNDS4[0]), min_y=float(BOUNDS4[2]),
                grid_w_inv=GRID_W_INV, grid_h_inv=GRID_H_INV, scale_factors=SCALE_FACTORS, inv_level_sigma2=INV_SIGMA2,
                log_scale_factor=float(LOG_SCALE), K4=K4, mbf=float(MBF), bounds4=BOUNDS4, q_cw=q, tcw=tcw, Ow=np.asarray(Ow, f32))


def world(kf, u, v, z):
    """World points (f32) that project near (u, v) at camera depth z in `kf`."""
    Rm = _rot64(kf["q_cw"])
    u, v = np.atleast_1d(np.asarray(u, np.float64)), np.atleast_1d(np.asarray(v, np.float64))
    z = np.broadcast_to(np.asarray(z, np.float64), u.shape)
    xc = np.stack([(u - float(K4[2])) * z / float(K4[0]), (v - float(K4[3])) * z / float(K4[1]), z], -1)
    return ((xc - kf["tcw"].astype(np.float64)) @ Rm).astype(f32)


def _flip(rng, d, nbits):
    d = np.array(d, np.uint8).copy()
    for b in rng.choice(256, nbits, replace=False):
        d[b // 8] ^= np.uint8(1 << (b % 8))
    return d


def _point_for(kf, u, v, z, level, desc):
    """(pos, normal, min_dist, max_dist, desc) of a map point at (u, v, z) of `kf`, seen head-on, whose predicted level there is `level`."""
    pos = world(kf, u, v, z)[0]
    PO = pos.astype(np.float64) - kf["Ow"].astype(np.float64)
    dist = np.linalg.norm(PO)
    max_dist = f32(dist * 1.2 ** (level - 0.5))          # log(max / dist) / log 1.2 = level - 0.5 -> ceil = level
    return pos, (PO / dist).astype(f32), f32(max_dist / 1.2 ** (N_LEVELS - 1)), max_dist, np.asarray(desc, np.uint8)


def _u_right(rng, x, z_fake):
    """mvuRight: -1 (none) for about half, x - mbf / depth for the rest."""
    return np.where(rng.random(len(x)) < 0.5, f32(-1), (x - MBF / z_fake).astype(f32)).astype(f32)


def _random_kf(rng, q, tcw, n, y_max=300.0):
    x = rng.uniform(12, W - 12, n).astype(f32)
    y = rng.uniform(12, y_max, n).astype(f32)
    depth = rng.uniform(1.0, 4.0, n).astype(f32)
    kf = make_kf(q, tcw, x, y, rng.integers(0, N_LEVELS, n), _u_right(rng, x, depth), rng.integers(0, 256, (n, 32), dtype=np.uint8))
    kf["depth"] = depth
    return kf


def _poses(K):
    return [(_quat([1.0, 2.0, 0.5 + 0.3 * k], 0.04 * k + 0.02), np.array([0.03 * k, -0.02 * k, 0.01 * k], f32)) for k in range(K)]


def _matching_points(rng, kfs, M, pts):
    """M map points, each the back-projection of a random key point of one of the key frames."""
    cand = [kf for kf in kfs if len(kf["x"])]
    if not cand and M:       # no key frame (or none with key points): the points of a key frame that is not handed on
        cand = [_random_kf(rng, *_poses(1)[0], 50)]
    for i in range(M):
        kf = cand[i % len(cand)]
        j = int(rng.integers(len(kf["x"])))
        pts.append(_point_for(kf, kf["x"][j], kf["y"][j], float(kf["depth"][j]), int(kf["octave"][j]), _flip(rng, kf["desc"][j], int(rng.integers(0, 30)))))


def _pack(pts):
    return dict(pos=np.array([p[0] for p in pts], f32).reshape(-1, 3), normal=np.array([p[1] for p in pts], f32).reshape(-1, 3),
                min_dist=np.array([p[2] for p in pts], f32), max_dist=np.array([p[3] for p in pts], f32),
                desc=np.array([p[4] for p in pts], np.uint8).reshape(-1, 32))


def _public(kfs):
    return [{k: v for k, v in kf.items() if k != "depth"} for kf in kfs]


def inputs():
    rng = np.random.default_rng(SEED)
    kfs = [_random_kf(rng, q, t, N_KP - (60 if k == 0 else 0)) for k, (q, t) in enumerate(_poses(3))]
    kf0 = kfs[0]
    # ---- the placed key points of key frame 0: (x, y, octave, u_right or None = consistent stereo, depth, descriptor)
    placed, where, pts = [], {}, []
    base = len(kf0["x"])

    def kp(x, y, octave, ur, desc=None, depth=2.0):
        placed.append((f32(x), f32(y), octave, f32(x - MBF / depth) if ur is None else f32(ur), depth,
                       rng.integers(0, 256, 32, dtype=np.uint8) if desc is None else desc))
        return base + len(placed) - 1

    def point(name, p):
        where.setdefault(name, []).append(len(pts))
        pts.append(p)

    lvl = 4
    sf = float(SCALE_FACTORS[lvl])
    D = lambda j: placed[j - base][5]
    j = kp(60, 340, lvl, -1);        point("candidate_mono", _point_for(kf0, 60, 340, 2.0, lvl, _flip(rng, D(j), 5)))
    j = kp(120, 340, lvl, None);     point("candidate_stereo", _point_for(kf0, 120, 340, 2.0, lvl, _flip(rng, D(j), 5)))
    j = kp(180, 340, lvl - 2, -1);   point("below_level", _point_for(kf0, 180, 340, 2.0, lvl, D(j)))
    j = kp(240, 340, lvl + 1, -1);   point("above_level", _point_for(kf0, 240, 340, 2.0, lvl, D(j)))
    j = kp(300 + 2.8 * sf, 340, lvl, -1);                 point("mono_gate", _point_for(kf0, 300, 340, 2.0, lvl, D(j)))
    j = kp(360, 340, lvl, 360 - float(MBF) / 2.0 + 2.9 * sf);    point("stereo_gate", _point_for(kf0, 360, 340, 2.0, lvl, D(j)))
    j = kp(420, 340, lvl, 0.0);      point("u_right_zero", _point_for(kf0, 420, 340, 2.0, lvl, D(j)))
    j = kp(480, 340, lvl, -1);       point("above_th_low", _point_for(kf0, 480, 340, 2.0, lvl, _flip(rng, D(j), 70)))
    j = kp(540, 340, lvl - 1, -1);   point("candidate_level_minus_1", _point_for(kf0, 540, 340, 2.0, lvl, _flip(rng, D(j), 2)))
    # a tie: A (the HIGHER index) in grid column 30, B in column 31, both 3 bits from the point's descriptor
    tie_desc = rng.integers(0, 256, 32, dtype=np.uint8)
    jb = kp(309, 400, lvl, -1, _flip(rng, tie_desc, 3))
    kp(60, 400, 0, -1)                                                      # (someone between the two indices)
    ja = kp(301, 400, lvl, -1, _flip(rng, tie_desc, 3))
    point("tie", _point_for(kf0, 305, 400, 2.0, lvl, tie_desc))
    where["tie_indices"] = [ja, jb]
    # windows clipped at each edge of the grid, with a key point to find
    # (a key point beyond 634.9 / 474.9 rounds to column 64 / row 48 and is in no cell at all)
    for name, (x, y) in dict(clip_left=(3, 420), clip_right=(W - 6, 420), clip_top=(200, 3), clip_bottom=(200, H - 6)).items():
        j = kp(x, y, lvl, -1)
        point(name, _point_for(kf0, x, y, 2.0, lvl, _flip(rng, D(j), 4)))
    point("empty_window", _point_for(kf0, 600, 400, 2.0, lvl, rng.integers(0, 256, 32, dtype=np.uint8)))
    # ---- the placed points that never reach a window
    rd = lambda: rng.integers(0, 256, 32, dtype=np.uint8)
    point("behind", _point_for(kf0, 320, 240, -1.5, 3, rd()))
    point("outside", _point_for(kf0, -40, 240, 2.0, 3, rd()))
    point("outside", _point_for(kf0, 320, H + 30, 2.0, 3, rd()))
    p = list(_point_for(kf0, 200, 200, 2.0, 3, rd())); p[2] = f32(p[3] * 2); point("too_near", tuple(p))
    p = list(_point_for(kf0, 220, 200, 2.0, 3, rd())); p[3] = f32(p[3] / 4); p[2] = f32(p[3] / 4); point("too_far", tuple(p))
    p = list(_point_for(kf0, 240, 200, 2.0, 3, rd())); p[1] = (-p[1]).astype(f32); point("view_angle", tuple(p))
    # z == +0.0f: q * special + tcw == 0 in the reference's own f32 sequence needs a pose made for it — key frame 2's translation is
    # rebuilt as -(q * special), and a neighbour with x != 0 found by search
    from tests.track_motion_restatement import se3_act
    special = np.array([0.4, -0.3, 0.2], f32)
    kf2 = kfs[2]
    with np.errstate(all="ignore"):
        kf2["tcw"] = (-se3_act(kf2["q_cw"], np.zeros(3, f32), special)[0]).astype(f32)
    kf2["Ow"] = (-(_rot64(kf2["q_cw"]).T @ kf2["tcw"].astype(np.float64))).astype(f32)
    point("z_zero_nan", (special, np.array([0, 0, 1], f32), f32(0.0), f32(10.0), rd()))
    g = (special.astype(np.float64) + _rot64(kf2["q_cw"]).T @ np.array([0.25, 0.1, 0.0])).astype(f32)
    grid = np.array([(g[0], L._ulps(g[1], a), L._ulps(g[2], b)) for a in range(-60, 61) for b in range(-60, 61)], f32)
    with np.errstate(all="ignore"):
        pc = se3_act(kf2["q_cw"], kf2["tcw"], grid)
    hit = np.flatnonzero((pc[:, 2] == 0) & ~np.signbit(pc[:, 2]) & (pc[:, 0] != 0))
    assert len(hit), "no float with a zero depth within 60 ulps"
    point("z_zero_inf", (np.ascontiguousarray(grid[hit[0]]), np.array([0, 0, 1], f32), f32(0.0), f32(10.0), rd()))
    # the camera centre of key frame 1 as a map point: in front of key frame 0; in key frame 1 itself the depth is tiny and the image
    # test rejects the pair before dist3D == 0 is met (no consistent pose reaches a zero distance: tests/test_orb_fuse.py hands one in)
    kfs[1]["Ow"] = np.array([0.05, 0.02, 1.5], f32)
    kfs[1]["tcw"] = (-(_rot64(kfs[1]["q_cw"]) @ kfs[1]["Ow"].astype(np.float64))).astype(f32)
    point("camera_centre", (kfs[1]["Ow"].copy(), np.array([0, 0, 1], f32), f32(0.0), f32(10.0), rd()))
    n_placed = len(pts)
    # key frame 0 with its placed key points
    px = [p[0] for p in placed]
    kfs[0] = dict(make_kf(kf0["q_cw"], kf0["tcw"], np.concatenate([kf0["x"], px]), np.concatenate([kf0["y"], [p[1] for p in placed]]),
                          np.concatenate([kf0["octave"], [p[2] for p in placed]]), np.concatenate([kf0["u_right"], [p[3] for p in placed]]),
                          np.concatenate([kf0["desc"], np.array([p[5] for p in placed], np.uint8)])),
                  depth=np.concatenate([kf0["depth"], np.array([p[4] for p in placed], f32)]))
    _matching_points(rng, kfs, 104 - n_placed - 6, pts)
    for name in ("skip_null", "skip_bad", "skip_in_kf"):
        where[name] = [len(pts), len(pts) + 1]
        _matching_points(rng, kfs, 2, pts)
    M = len(pts)
    skip = np.zeros((3, M), np.uint8)
    for code, name in ((1, "skip_null"), (2, "skip_bad")):
        skip[:, where[name]] = code                     # for every key frame
    skip[0, where["skip_in_kf"][0]] = 3                 # in one key frame only
    skip[2, where["skip_in_kf"][1]] = 3
    return dict(kfs=_public(kfs), points=_pack(pts), skip=skip, th=TH, where=where)


def random_inputs(K=3, M=300, N=300, seed=1, empty_kf=None, y_max=H - 12.0):
    """K key frames of N key points (key frame `empty_kf` of none), M matching points, a sprinkle of skipped pairs."""
    rng = np.random.default_rng(SEED + seed)
    kfs = [_random_kf(rng, q, t, 0 if k == empty_kf else N, y_max) for k, (q, t) in enumerate(_poses(K))]
    pts = []
    _matching_points(rng, kfs, M, pts)
    skip = (rng.random((K, M)) < 0.05).astype(np.uint8)
    return dict(kfs=_public(kfs), points=_pack(pts), skip=skip, th=TH, where={})


def crowd_inputs(n=200):
    """One key frame whose `n` key points all lie inside the window of every point (level 7: radius 3 * 1.2^7 = 10.7 px, one grid
    cell is 10 px: a column's range exceeds 64 members), with descriptors from a pool of four so that equal distances lie on both
    sides of a 64-member stride; 8 points at the crowd's centre, each a few bits from one pool descriptor."""
    rng = np.random.default_rng(SEED + 77)
    q, t = _poses(1)[0]
    lvl = N_LEVELS - 1
    x = (f32(322.0) + rng.uniform(-1.5, 1.5, n)).astype(f32)        # one or two columns of the grid
    y = (f32(241.0) + rng.uniform(-8.0, 8.0, n)).astype(f32)
    pool = rng.integers(0, 256, (4, 32), dtype=np.uint8)
    desc = pool[rng.integers(0, 4, n)]
    octave = np.where(rng.random(n) < 0.8, lvl, lvl - 1)
    kf = make_kf(q, t, x, y, octave, np.where(rng.random(n) < 0.5, f32(-1), (x - MBF / f32(2.0)).astype(f32)), desc)
    pts = [_point_for(kf, 322.0 + dx, 241.0, 2.0, lvl, _flip(rng, pool[i % 4], i // 4)) for i, dx in enumerate(np.linspace(-1, 1, 8))]
    return dict(kfs=[kf], points=_pack(pts), skip=None, th=TH, where={})


def ambiguous_inputs():
    """random_inputs(2, 65, 200) with max_dist = float(dist3D * 1.2^k) for the first 24 points in key frame 0: the quotient
    log(ratio) / log(1.2) lies within eps of the integer k."""
    inp = random_inputs(2, 65, 200, seed=5)
    fr = R.front(inp["kfs"][0], inp["points"])
    for i in range(24):
        k = 1 + i % 6
        inp["points"]["max_dist"][i] = f32(float(fr["dist"][i]) * 1.2 ** k)
        inp["points"]["min_dist"][i] = f32(inp["points"]["max_dist"][i] / 1.2 ** 7)
    return inp


def digest(inp):
    h = hashlib.sha1()
    for kf in inp["kfs"]:
        for k in ("x", "y", "octave", "u_right", "desc", "scale_factors", "inv_level_sigma2", "K4", "bounds4", "q_cw", "tcw", "Ow"):
            h.update(np.ascontiguousarray(kf[k]).tobytes())
        h.update(np.array([kf["min_x"], kf["min_y"], kf["grid_w_inv"], kf["grid_h_inv"], kf["log_scale_factor"], kf["mbf"]], f32).tobytes())
    for k in ("pos", "normal", "min_dist", "max_dist", "desc"):
        h.update(np.ascontiguousarray(inp["points"][k]).tobytes())
    if inp["skip"] is not None:
        h.update(np.ascontiguousarray(inp["skip"]).tobytes())
    h.update(np.array([inp["th"]], f32).tobytes())
    return h.hexdigest()


def views(inp):
    """-> (list of orbmatcher.FuseKeyFrame, orbmatcher.FusePoints)."""
    from plvs_amd.orbmatcher import FrameView, FuseKeyFrame, FusePoints
    kfs = [FuseKeyFrame(FrameView(kf["x"], kf["y"], kf["octave"], kf["u_right"], kf["desc"], kf["min_x"], kf["min_y"], kf["grid_w_inv"],
                                  kf["grid_h_inv"], kf["scale_factors"]), kf["inv_level_sigma2"], kf["log_scale_factor"], kf["K4"], kf["mbf"],
                        kf["bounds4"], kf["q_cw"], kf["tcw"], kf["Ow"]) for kf in inp["kfs"]]
    p = inp["points"]
    return kfs, FusePoints(p["pos"], p["normal"], p["min_dist"], p["max_dist"], p["desc"])
