"""Seeded scenario behind tests/golden/track_local_reference.npz: a 640 x 480 frame (TUM1 intrinsics, no distortion, 8 point
levels and 3 line levels at 1.2) of about 350 key points and 80 key lines, half of them with stereo coordinates, and a local map
of about 600 points and 120 lines seen from a pose that is not the identity — for Frame::isInFrustum over the local map and the
two searches behind it (Tracking::SearchLocalPoints / SearchLocalLines).  Most map elements are key points / key lines
back-projected at a chosen depth with a few descriptor bits flipped: they match.  The rest are placed cases, listed in
inputs()["where"]: behind the camera, outside each of the four bounds, PcZ == 0 exactly, too near and too far (lines: inside the
band a MapLine with mfMinDistance would have, which the reference's 0.8f * mfMaxDistance rejects), grazing normals on both sides
of 0.5, viewCos on both sides of 0.998, levels clamped at 0 and at the top, points beyond the far-point cut, skipped elements, a
line with an end point behind the camera, and points / lines whose ratio is the f32 nearest to 1.2^k and its neighbours.
crowd_inputs() is a second, separate set: 200 map points over one cluster of 300 key points (more candidates than the window
launch's first capacity).  scripts/make_track_local_golden.py asserts each on the reference's run."""
import hashlib

import numpy as np

from tests import track_local_restatement as R
from tests.frame_rgbd_scenario import KEYLINE_DTYPE

f32 = np.float32
SEED = 20241019
W, H = 640, 480
K4 = np.array([517.306408, 516.469215, 318.643040, 255.313989], f32)      # TUM1.yaml: fx, fy, cx, cy
MBF = f32(40.0)
BOUNDS4 = np.array([0, W, 0, H], f32)
N_LEVELS, N_LINE_LEVELS = 8, 3
SCALE = f32(1.2)
VIEWING_COS_LIMIT = f32(0.5)
TH_FAR = f32(6.0)
NN_RATIO = 0.8


def _scale_factors(n):
    s = [f32(1.0)]
    for _ in range(1, n):
        s.append(f32(s[-1] * SCALE))
    return np.array(s, f32)


SCALE_FACTORS = _scale_factors(N_LEVELS)
LINE_SCALE_FACTORS = _scale_factors(N_LINE_LEVELS)
LINE_INV_SIGMA2 = (f32(1.0) / (LINE_SCALE_FACTORS * LINE_SCALE_FACTORS)).astype(f32)
LOG_SCALE = f32(np.log(np.float64(SCALE)))          # mfLogScaleFactor = log(mfScaleFactor)
MAX_DIAG = float(f32(np.sqrt(f32(W * W + H * H))))
GRID_W_INV, GRID_H_INV = float(f32(64.0) / f32(W)), float(f32(48.0) / f32(H))


def _pose(special):
    """Rcw (column-major 9), tcw, Ow of a camera rotated by 0.25 rad about (1, 2, 0.5) and moved; tcw[2] is chosen so that the
    world point `special` has PcZ == 0 exactly in the reference's f32 sequence."""
    a = np.array([1.0, 2.0, 0.5])
    a /= np.linalg.norm(a)
    ang = 0.25
    Kx = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    Rm = (np.eye(3) + np.sin(ang) * Kx + (1 - np.cos(ang)) * Kx @ Kx).astype(f32)
    Rcw = np.ascontiguousarray(Rm.T.reshape(-1))      # column-major: R(r, c) = Rcw[3 c + r]
    x, y, z = (f32(v) for v in special)
    t2 = -f32(Rcw[2] * x + f32(Rcw[5] * y + Rcw[8] * z))
    tcw = np.array([0.3, -0.2, t2], f32)
    Ow = (-(Rm.astype(np.float64).T @ tcw.astype(np.float64))).astype(f32)
    return Rcw, tcw, Ow, Rm.astype(np.float64)


def camera(special=(0.4, -0.3, 0.2)):
    Rcw, tcw, Ow, _ = _pose(special)
    return dict(K4=K4, mbf=MBF, bounds4=BOUNDS4, Rcw=Rcw, tcw=tcw, Ow=Ow, viewing_cos_limit=VIEWING_COS_LIMIT, log_scale_factor=LOG_SCALE,
                n_levels=N_LEVELS, line_log_scale_factor=LOG_SCALE, n_line_levels=N_LINE_LEVELS)


def _world(cam, u, v, z):
    """World point (f32) that projects near (u, v) at camera depth z."""
    Rm = np.asarray(cam["Rcw"], np.float64).reshape(3, 3).T
    xc = np.stack([(u - float(K4[2])) * z / float(K4[0]), (v - float(K4[3])) * z / float(K4[1]), z * np.ones_like(u)], -1)
    return ((xc - cam["tcw"].astype(np.float64)) @ Rm).astype(f32)       # R^T (xc - t)


def _view_normal(cam, p, tilt_deg=0.0, rng=None):
    """Unit vector at `tilt_deg` from the viewing ray Ow -> p (viewCos = cos tilt)."""
    d = p.astype(np.float64) - cam["Ow"].astype(np.float64)
    d /= np.linalg.norm(d)
    if tilt_deg == 0.0:
        return d.astype(f32)
    o = np.cross(d, [0.0, 0.0, 1.0])
    o /= np.linalg.norm(o)
    t = np.deg2rad(tilt_deg)
    return (np.cos(t) * d + np.sin(t) * o).astype(f32)


def _dist(cam, p):
    return R._norm((np.asarray(p, f32).reshape(1, 3) - cam["Ow"][None, :]).astype(f32))[0]


def _max_for_ratio(dist, target):
    """mfMaxDistance (f32) with f32(max / dist) == target exactly, searched around target * dist."""
    base = f32(target * dist)
    for step in range(0, 64):
        for sgn in (1, -1):
            c = base
            for _ in range(step):
                c = np.nextafter(c, f32(np.inf) if sgn > 0 else f32(-np.inf), dtype=f32)
            if f32(c / dist) == target:
                return c
    return None          # (the quotients of this dist step over the target: the caller takes another element)


def _ulps(x, k):
    for _ in range(abs(k)):
        x = np.nextafter(x, f32(np.inf) if k > 0 else f32(-np.inf), dtype=f32)
    return f32(x)


def _flip(rng, d, nbits):
    out = d.copy()
    for b in rng.permutation(256)[:nbits]:
        out[b // 8] ^= np.uint8(1 << (b % 8))
    return out


def _frame(rng, n_kp, n_kl):
    x, y = rng.uniform(8, W - 8, n_kp).astype(f32), rng.uniform(8, H - 8, n_kp).astype(f32)
    octave = rng.integers(0, N_LEVELS, n_kp).astype(np.int32)
    desc = rng.integers(0, 256, (n_kp, 32), dtype=np.uint8)
    depth = rng.uniform(1.0, 8.0, n_kp)
    u_right = np.where(np.arange(n_kp) % 2 == 0, x - float(MBF) / depth, -1).astype(f32)
    kl = np.zeros(n_kl, KEYLINE_DTYPE)
    cx, cy = rng.uniform(80, W - 80, n_kl), rng.uniform(80, H - 80, n_kl)
    ang, ln = rng.uniform(-np.pi, np.pi, n_kl), rng.uniform(30, 120, n_kl)
    kl["startPointX"], kl["startPointY"] = cx - 0.5 * ln * np.cos(ang), cy - 0.5 * ln * np.sin(ang)
    kl["endPointX"], kl["endPointY"] = cx + 0.5 * ln * np.cos(ang), cy + 0.5 * ln * np.sin(ang)
    kl["angle"] = np.arctan2(kl["endPointY"] - kl["startPointY"], kl["endPointX"] - kl["startPointX"])
    kl["octave"] = rng.integers(0, N_LINE_LEVELS, n_kl)
    kl["lineLength"] = ln
    ldesc = rng.integers(0, 256, (n_kl, 32), dtype=np.uint8)
    ldepth = rng.uniform(1.5, 6.0, (n_kl, 2))
    stereo = np.arange(n_kl) % 2 == 0
    urs = np.where(stereo, kl["startPointX"] - float(MBF) / ldepth[:, 0], -1).astype(f32)
    ure = np.where(stereo, kl["endPointX"] - float(MBF) / ldepth[:, 1], -1).astype(f32)
    return dict(x=x, y=y, octave=octave, desc=desc, u_right=u_right, depth=depth, keylines=kl, line_desc=ldesc, line_depth=ldepth,
                u_right_start=urs, u_right_end=ure)


class _Points:
    def __init__(self):
        self.pos, self.normal, self.min_dist, self.max_dist, self.desc, self.skip = [], [], [], [], [], []

    def add(self, pos, normal, min_dist, max_dist, desc, skip=0):
        self.pos.append(np.asarray(pos, f32)); self.normal.append(np.asarray(normal, f32))
        self.min_dist.append(f32(min_dist)); self.max_dist.append(f32(max_dist)); self.desc.append(desc); self.skip.append(skip)
        return len(self.pos) - 1

    def arrays(self, rng):
        m = len(self.pos)
        return dict(skip=np.array(self.skip, np.uint8), pos=np.array(self.pos, f32).reshape(m, 3), normal=np.array(self.normal, f32).reshape(m, 3),
                    min_dist=np.array(self.min_dist, f32), max_dist=np.array(self.max_dist, f32), desc=np.array(self.desc, np.uint8).reshape(m, 32),
                    has_obs=(rng.random(m) < 0.95).astype(np.uint8))


def inputs():
    rng = np.random.default_rng(SEED)
    cam = camera()
    fr = _frame(rng, 350, 80)
    where = {}
    P = _Points()
    top = float(SCALE) ** (N_LEVELS - 1)

    def matching_point(i, tilt=0.0, level_shift=None, z=None, du=0.0):
        z = fr["depth"][i] if z is None else z
        p = _world(cam, fr["x"][i:i + 1].astype(np.float64) + du, fr["y"][i:i + 1].astype(np.float64), z)[0]
        d = float(_dist(cam, p))
        shift = rng.choice([-0.3, 0.5]) if level_shift is None else level_shift        # predicted level = octave or octave + 1
        mx = d * float(SCALE) ** (fr["octave"][i] + shift)
        return P.add(p, _view_normal(cam, p, tilt), mx / top, mx, _flip(rng, fr["desc"][i], int(rng.integers(0, 24))))

    # ---- the map points that match: most key points once, with a small tilt of the normal
    order = [int(i) for i in rng.permutation(350)]
    for i in order[:270]:
        matching_point(i, tilt=float(rng.uniform(0, 3.0)))
    # ---- placed cases, on the key points no other map point claims
    free = order[270:]
    where["view_cos_above_998"] = [matching_point(free.pop(), tilt=3.0) for _ in range(4)]
    where["view_cos_below_998"] = [matching_point(free.pop(), tilt=4.5) for _ in range(4)]
    where["grazing_kept"] = [matching_point(free.pop(), tilt=59.0) for _ in range(3)]
    where["grazing_rejected"] = [matching_point(free.pop(), tilt=61.0) for _ in range(3)]
    # projections beside their key point: found only by a window th times as wide (the radius is 2.5 or 4 px times th times the level's scale)
    low = [i for i in free if fr["octave"][i] <= 4 and 80 < fr["x"][i] < W - 80]
    shifted = lambda i, f: matching_point(i, du=f * 2.5 * float(SCALE_FACTORS[fr["octave"][i]]), level_shift=-0.3)      # level = octave
    where["needs_th3"] = [shifted(low.pop(), 2.0) for _ in range(4)]
    where["needs_th15"] = [shifted(low.pop(), 8.0) for _ in range(4)]
    taken = set(fr_i for fr_i in free if fr["octave"][fr_i] <= 4 and 80 < fr["x"][fr_i] < W - 80) - set(low)
    free = [i for i in free if i not in taken]
    where["far_cut"] = [matching_point(free.pop(), z=float(rng.uniform(6.5, 7.9))) for _ in range(6)]

    def free_point(u, v, z, min_dist=None, max_dist=None, tilt=0.0):
        p = _world(cam, np.array([u], np.float64), np.array([v], np.float64), z)[0]
        d = float(_dist(cam, p))
        mx = d * 1.5 if max_dist is None else max_dist(d)
        mn = mx / top if min_dist is None else min_dist(d)
        return P.add(p, _view_normal(cam, p, tilt), mn, mx, rng.integers(0, 256, 32, dtype=np.uint8))

    where["behind"] = [free_point(rng.uniform(100, 500), rng.uniform(100, 400), -rng.uniform(0.5, 4.0)) for _ in range(8)]
    where["out_left"] = [free_point(-rng.uniform(5, 200), rng.uniform(50, 430), rng.uniform(1, 5)) for _ in range(5)]
    where["out_right"] = [free_point(W + rng.uniform(5, 200), rng.uniform(50, 430), rng.uniform(1, 5)) for _ in range(5)]
    where["out_top"] = [free_point(rng.uniform(50, 590), -rng.uniform(5, 200), rng.uniform(1, 5)) for _ in range(5)]
    where["out_bottom"] = [free_point(rng.uniform(50, 590), H + rng.uniform(5, 200), rng.uniform(1, 5)) for _ in range(5)]
    where["pcz_zero"] = [P.add(np.array([0.4, -0.3, 0.2], f32), np.array([0, 0, 1], f32), 0.1, 10.0, rng.integers(0, 256, 32, dtype=np.uint8))]
    where["too_near"] = [free_point(rng.uniform(50, 590), rng.uniform(50, 430), rng.uniform(1, 5), min_dist=lambda d: d * 1.3, max_dist=lambda d: d * 4)
                         for _ in range(6)]          # 0.8f * min = 1.04 d > d
    where["too_far"] = [free_point(rng.uniform(50, 590), rng.uniform(50, 430), rng.uniform(1, 5), max_dist=lambda d: d * 0.8) for _ in range(6)]
    where["level_clamped_0"] = [free_point(rng.uniform(50, 590), rng.uniform(50, 430), rng.uniform(1, 5), max_dist=lambda d: d * 0.9) for _ in range(5)]
    where["level_clamped_top"] = [free_point(rng.uniform(50, 590), rng.uniform(50, 430), rng.uniform(1, 5), min_dist=lambda d: d * 0.01,
                                             max_dist=lambda d: d * float(SCALE) ** 9.4) for _ in range(5)]
    # ---- ratio = the f32 nearest to 1.2^k, and its neighbours: the logarithm's last bit decides the level
    where["ratio_points"] = []
    for k in range(1, 7):
        target = f32(np.exp(k * np.float64(LOG_SCALE)))
        for off in (-1, 0, 1):
            mx = None
            while mx is None:
                i = free.pop()
                p = _world(cam, fr["x"][i:i + 1].astype(np.float64), fr["y"][i:i + 1].astype(np.float64), fr["depth"][i])[0]
                mx = _max_for_ratio(_dist(cam, p), _ulps(target, off))
            idx = P.add(p, _view_normal(cam, p), float(mx) / top / 1.5, mx, _flip(rng, fr["desc"][i], 5))
            where["ratio_points"].append((idx, k, off))
    # ---- the rest: points around the frustum, in and out
    while len(P.pos) < 600:
        free_point(rng.uniform(-100, W + 100), rng.uniform(-100, H + 100), rng.uniform(-1, 7), max_dist=lambda d: d * float(rng.uniform(0.7, 5.0)),
                   tilt=float(rng.uniform(0, 80)))
    points = P.arrays(rng)
    skipped = rng.permutation(600)[:30]
    placed = {i for v in where.values() for i in (x[0] if isinstance(x, tuple) else x for x in v)}
    skipped = np.array([s for s in skipped if int(s) not in placed])
    points["skip"][skipped] = 1
    where["skipped_points"] = [int(s) for s in skipped]

    # ---- map lines
    kl = fr["keylines"]
    Ls = dict(skip=[], start=[], end=[], normal=[], max_dist=[], min_dist=[], desc=[])

    def add_line(s, e, max_of, desc, tilt=0.0, min_of=None, skip=0):
        mid = (f32(0.5) * (s + e)).astype(f32)
        d = float(_dist(cam, mid))
        mx = max_of(d)
        Ls["skip"].append(skip); Ls["start"].append(s); Ls["end"].append(e); Ls["normal"].append(_view_normal(cam, mid, tilt))
        Ls["max_dist"].append(f32(mx)); Ls["min_dist"].append(f32(mx / 1.44 if min_of is None else min_of(d))); Ls["desc"].append(desc)
        return len(Ls["skip"]) - 1

    def line_of(j, zs=None, ze=None):
        zs = fr["line_depth"][j, 0] if zs is None else zs
        ze = fr["line_depth"][j, 1] if ze is None else ze
        s = _world(cam, np.array([kl["startPointX"][j]], np.float64), np.array([kl["startPointY"][j]], np.float64), zs)[0]
        e = _world(cam, np.array([kl["endPointX"][j]], np.float64), np.array([kl["endPointY"][j]], np.float64), ze)[0]
        return s, e

    for j in range(80):        # every key line once: level = its octave or one above (ratio in [1 / 1.2, 1.25])
        o = int(kl["octave"][j])
        r = {0: rng.uniform(0.86, 0.98), 1: rng.uniform(1.02, 1.18), 2: rng.uniform(1.21, 1.24)}[o if rng.random() < 0.6 else min(o + 1, 2)]
        add_line(*line_of(j), lambda d, r=r: d * r, _flip(rng, fr["line_desc"][j], int(rng.integers(0, 30))), tilt=float(rng.uniform(0, 10)))
    lfree = [int(j) for j in rng.permutation(80)]
    rnd = lambda: rng.integers(0, 256, 32, dtype=np.uint8)
    where["line_near_quirk"] = [add_line(*line_of(lfree.pop()), lambda d: d * 1.35, rnd(), min_of=lambda d: d * 0.9) for _ in range(4)]   # 0.72 min <= d < 0.8 max
    where["line_too_far"] = [add_line(*line_of(lfree.pop()), lambda d: d * 0.8, rnd()) for _ in range(4)]
    where["line_grazing_kept"] = [add_line(*line_of(lfree.pop()), lambda d: d, rnd(), tilt=59.0) for _ in range(2)]
    where["line_grazing_rejected"] = [add_line(*line_of(lfree.pop()), lambda d: d, rnd(), tilt=61.0) for _ in range(2)]
    j = lfree.pop()
    where["line_end_behind"] = [add_line(*line_of(j, zs=3.0, ze=-0.8), lambda d: d * 1.1, rnd())]
    where["line_behind"] = [add_line(*line_of(lfree.pop(), zs=-2.0, ze=-3.0), lambda d: d, rnd()) for _ in range(3)]

    def outside_line(u, v):
        s = _world(cam, np.array([u], np.float64), np.array([v], np.float64), 3.0)[0]
        e = _world(cam, np.array([u + 20.0], np.float64), np.array([v + 20.0], np.float64), 3.2)[0]
        return add_line(s, e, lambda d: d, rnd())

    where["line_outside"] = [outside_line(-150.0, 200.0), outside_line(W + 150.0, 200.0), outside_line(300.0, -150.0), outside_line(300.0, H + 150.0)]
    where["ratio_lines"] = []
    target = f32(np.exp(np.float64(LOG_SCALE)))
    for off in (-1, 0, 1):
        mx = None
        while mx is None:
            j = lfree.pop()
            s, e = line_of(j)
            mid = (f32(0.5) * (s + e)).astype(f32)
            mx = _max_for_ratio(_dist(cam, mid), _ulps(target, off))
        where["ratio_lines"].append((add_line(s, e, lambda d, mx=mx: mx, _flip(rng, fr["line_desc"][j], 5)), 1, off))
    j = lfree.pop()
    s, e = line_of(j)
    where["ratio_lines"].append((add_line(s, e, lambda d, s=s, e=e: _dist(cam, (f32(0.5) * (s + e)).astype(f32)), _flip(rng, fr["line_desc"][j], 5)), 0, 0))
    while len(Ls["skip"]) < 120:
        add_line(*line_of(int(rng.integers(0, 80)), zs=float(rng.uniform(-1, 6)), ze=float(rng.uniform(-1, 6))),
                 lambda d: d * float(rng.uniform(0.7, 1.5)), rnd(), tilt=float(rng.uniform(0, 80)))
    ml = len(Ls["skip"])
    lines = dict(skip=np.array(Ls["skip"], np.uint8), start=np.array(Ls["start"], f32).reshape(ml, 3), end=np.array(Ls["end"], f32).reshape(ml, 3),
                 normal=np.array(Ls["normal"], f32).reshape(ml, 3), max_dist=np.array(Ls["max_dist"], f32), min_dist=np.array(Ls["min_dist"], f32),
                 desc=np.array(Ls["desc"], np.uint8).reshape(ml, 32), has_obs=(rng.random(ml) < 0.9).astype(np.uint8))
    lines["skip"][[109, 113, 118]] = 1          # (among the random tail)
    where["skipped_lines"] = [109, 113, 118]
    frame = dict(x=fr["x"], y=fr["y"], octave=fr["octave"], u_right=fr["u_right"], desc=fr["desc"], keylines=kl, line_desc=fr["line_desc"],
                 u_right_start=fr["u_right_start"], u_right_end=fr["u_right_end"],
                 occupied_points=(rng.random(350) < 0.08).astype(np.uint8), occupied_lines=(rng.random(80) < 0.08).astype(np.uint8))
    return dict(cam=cam, frame=frame, points=points, lines=lines, where=where)


def crowd_inputs():
    """200 map points over one cluster of 300 key points at the two top octaves: every point's window holds the whole cluster,
    60 000 candidates against a first capacity of 200 * 32 + 4096."""
    rng = np.random.default_rng(SEED + 1)
    cam = camera()
    n, m = 300, 200
    x, y = (320 + rng.uniform(-6, 6, n)).astype(f32), (240 + rng.uniform(-6, 6, n)).astype(f32)
    octave = rng.integers(6, 8, n).astype(np.int32)
    base = rng.integers(0, 256, 32, dtype=np.uint8)
    desc = np.array([_flip(rng, base, int(rng.integers(0, 60))) for _ in range(n)], np.uint8)
    depth = rng.uniform(2.0, 4.0, n)
    u_right = np.where(np.arange(n) % 3 == 0, x - float(MBF) / depth, -1).astype(f32)
    P = _Points()
    for k in range(m):
        i = int(rng.integers(0, n))
        p = _world(cam, x[i:i + 1].astype(np.float64), y[i:i + 1].astype(np.float64), depth[i])[0]
        d = float(_dist(cam, p))
        mx = d * float(SCALE) ** 6.5          # level 7
        P.add(p, _view_normal(cam, p, float(rng.uniform(0, 5))), mx / float(SCALE) ** 7, mx, _flip(rng, desc[i], int(rng.integers(0, 20))))
    points = P.arrays(rng)
    frame = dict(x=x, y=y, octave=octave, u_right=u_right, desc=desc, occupied_points=(rng.random(n) < 0.05).astype(np.uint8))
    return dict(cam=cam, frame=frame, points=points, lines=None, where={})


def random_inputs(m=3000, ml=300, seed=5, n_kp=1500, n_kl=300):
    """The timing set: a frame of n_kp key points and n_kl key lines, m map points and ml map lines around the frustum."""
    rng = np.random.default_rng(seed)
    cam = camera()
    fr = _frame(rng, n_kp, n_kl)
    kl = fr["keylines"]
    top = float(SCALE) ** (N_LEVELS - 1)
    src = rng.integers(0, n_kp, m)
    jit = rng.normal(0, 1.0, (m, 2))
    out = rng.random(m) < 0.3
    jit[out] += rng.normal(0, 400, (int(out.sum()), 2))
    pos = _world(cam, fr["x"][src] + jit[:, 0], fr["y"][src] + jit[:, 1], fr["depth"][src] * np.where(rng.random(m) < 0.05, -1, 1))
    dist = R._norm((pos - cam["Ow"][None, :]).astype(f32)).astype(np.float64)
    mx = dist * float(SCALE) ** (fr["octave"][src] + rng.choice([-0.3, 0.5], m)) * np.where(rng.random(m) < 0.1, 0.5, 1.0)
    normal = np.array([_view_normal(cam, p, float(t)) for p, t in zip(pos, rng.uniform(0, 70, m))], f32)
    pdesc = fr["desc"][src] ^ (rng.integers(0, 256, (m, 32), dtype=np.uint8) & rng.integers(0, 256, (m, 32), dtype=np.uint8)
                               & rng.integers(0, 256, (m, 32), dtype=np.uint8) & rng.integers(0, 256, (m, 32), dtype=np.uint8))
    points = dict(skip=(rng.random(m) < 0.05).astype(np.uint8), pos=pos, normal=normal, min_dist=(mx / top).astype(f32), max_dist=mx.astype(f32),
                  desc=pdesc, has_obs=(rng.random(m) < 0.95).astype(np.uint8))
    lsrc = rng.integers(0, n_kl, ml)
    zs, ze = fr["line_depth"][lsrc, 0], fr["line_depth"][lsrc, 1]
    start = _world(cam, kl["startPointX"][lsrc].astype(np.float64), kl["startPointY"][lsrc].astype(np.float64), zs)
    end = _world(cam, kl["endPointX"][lsrc].astype(np.float64), kl["endPointY"][lsrc].astype(np.float64), ze)
    mid = (f32(0.5) * (start + end)).astype(f32)
    ldist = R._norm((mid - cam["Ow"][None, :]).astype(f32)).astype(np.float64)
    lnormal = np.array([_view_normal(cam, p, float(t)) for p, t in zip(mid, rng.uniform(0, 70, ml))], f32)
    ldesc = fr["line_desc"][lsrc] ^ (rng.integers(0, 256, (ml, 32), dtype=np.uint8) & rng.integers(0, 256, (ml, 32), dtype=np.uint8)
                                     & rng.integers(0, 256, (ml, 32), dtype=np.uint8))
    lines = dict(skip=(rng.random(ml) < 0.05).astype(np.uint8), start=start, end=end, normal=lnormal,
                 max_dist=(ldist * rng.uniform(0.75, 1.3, ml)).astype(f32), desc=ldesc, has_obs=(rng.random(ml) < 0.9).astype(np.uint8))
    frame = dict(x=fr["x"], y=fr["y"], octave=fr["octave"], u_right=fr["u_right"], desc=fr["desc"], keylines=kl, line_desc=fr["line_desc"],
                 u_right_start=fr["u_right_start"], u_right_end=fr["u_right_end"],
                 occupied_points=(rng.random(n_kp) < 0.08).astype(np.uint8), occupied_lines=(rng.random(n_kl) < 0.08).astype(np.uint8))
    return dict(cam=cam, frame=frame, points=points, lines=lines, where={})


def prefix(inp, m, ml):
    """The first m map points and ml map lines of a set (the frame unchanged)."""
    out = dict(inp)
    out["points"] = {k: v[:m] for k, v in inp["points"].items()}
    out["lines"] = None if inp["lines"] is None else {k: v[:ml] for k, v in inp["lines"].items()}
    return out


def inputs_digest(inp):
    h = hashlib.sha1()
    cam = inp["cam"]
    for k in ("K4", "bounds4", "Rcw", "tcw", "Ow"):
        h.update(np.ascontiguousarray(cam[k], f32).tobytes())
    for k in ("mbf", "viewing_cos_limit", "log_scale_factor", "line_log_scale_factor"):
        h.update(f32(cam[k]).tobytes())
    h.update(np.array([cam["n_levels"], cam["n_line_levels"]], np.int32).tobytes())
    for part in ("frame", "points", "lines"):
        if inp[part] is not None:
            for k in sorted(inp[part]):
                h.update(np.ascontiguousarray(inp[part][k]).tobytes())
    return h.hexdigest()


def frame_view(inp):
    """orbmatcher.FrameView of a set's frame."""
    from plvs_amd.orbmatcher import FrameView
    fr = inp["frame"]
    return FrameView(fr["x"], fr["y"], fr["octave"], fr["u_right"], fr["desc"], 0.0, 0.0, GRID_W_INV, GRID_H_INV, SCALE_FACTORS)


def line_view(inp, n=None):
    """linematcher.line_frame_view of a set's frame (None without lines)."""
    from plvs_amd.linematcher import line_frame_view
    fr = inp["frame"]
    if "keylines" not in fr:
        return None
    s = slice(None, n)
    return line_frame_view(fr["keylines"][s], fr["line_desc"][s], LINE_SCALE_FACTORS, LINE_INV_SIGMA2, MAX_DIAG, fr["u_right_start"][s],
                           fr["u_right_end"][s], float(MBF))


def mappoint_view(points, fields):
    """orbmatcher.MapPointView of the frustum fields of a set's points (fields: p_* of the restatement / golden)."""
    from plvs_amd.orbmatcher import MapPointView
    m = len(points["skip"])
    return MapPointView(fields["p_in_view"], np.zeros(m, np.uint8), fields["p_proj_x"], fields["p_proj_y"], fields["p_proj_xr"], fields["p_view_cos"],
                        fields["p_track_depth"], fields["p_level"], points["desc"], points["has_obs"])


SEARCH_CASES = [(th, far, occ) for th in (1.0, 3.0, 15.0) for far in (False, True) for occ in (True, False)]
LINE_CASES = [(larger, occ) for larger in (False, True) for occ in (True, False)]


def search_key(th, far, occ):
    return f"assigned_points_th{int(th)}_far{int(far)}_occ{int(occ)}"


def line_key(larger, occ):
    return f"assigned_lines_larger{int(larger)}_occ{int(occ)}"
