"""Seeded scenario behind tests/golden/track_motion_reference.npz: a 640 x 480 frame (TUM1 intrinsics, 8 point levels and 3 line
levels at 1.2) of 200 key points and 40 key lines, half of them with stereo coordinates, and a last frame of about 100 map points
and 30 map lines seen from a current pose that is a rotation of 0.25 rad about (1, 2, 0.5) — for the search of
Tracking::TrackWithMotionModel (plvs_hip_frame_search_last_frame).  Most last-frame elements are key points / key lines of the
current frame back-projected at their depth with a few descriptor bits flipped: they match.  The rest are placed cases, listed in
inputs()["where"]; scripts/make_track_motion_golden.py asserts each on the reference's run.

Points: invalid; behind the camera; z == +0.0f exactly with x == y == 0 (a NaN projection, which the four comparisons accept) and
with x != 0 (an infinite one, rejected); outside each bound and exactly ON each bound (accepted); accepted at octave 0 and at the top
octave, with and without u_right; `mid` points beside their key point by 11 px times the
level's scale (found at th = 15, not at 7) and `wide` ones by 1.5 radii of th = 15 (found only at 2 * th).  The translation is
-(q * special), so the world point `special` is the camera centre in the reference's own f32 sequence.
z == -0.0f (invz = -inf, rejected by `invzc < 0`) needs signed zeros in the pose and has a small set of its own, minus_zero_inputs():
a half turn about z, q = (0, 1e-30, -1, 0) with tcw = (0, 0, -0.0f), takes p = (1, 0, -0.0f) to (-1, 0, -0.0f) — every term of the
last coefficient is a -0 (a product of a zero or an underflowing factor carries a sign) — and the same point with p(2) = +0.0f to
z == +0.0f, beside points it accepts and matches.

Lines: invalid; middle behind; middle outside each bound; too near, too far, and exactly on both edges of [0.8f, 1.2f] *
mfMaxDistance with the neighbouring float outside; start behind with the middle in front, end behind; start out of bounds, end out
of bounds; `shifted` lines 2.1 px beside their key line (octave 0), inside the larger chi-square gate only.

Three last-frame poses give bForward, bBackward and neither.  policy_inputs() cuts the valid sets so that the retry rules run:
"few_points" (the first search finds fewer than 20, the second at 2 * th finds the wide ones), "few_lines" (points pass, lines find
fewer than 10 until the larger gate), "plain" (neither).  crowd_inputs(): 200 last-frame points over one cluster of 300 key points
(more candidates than the window launch's first capacity)."""
import hashlib

import numpy as np

from tests import track_local_scenario as L
from tests import track_motion_restatement as R

f32 = np.float32
SEED = 20261019
W, H, K4, MBF, BOUNDS4 = L.W, L.H, L.K4, L.MBF, L.BOUNDS4
MB = f32(0.08)
N_LEVELS, N_LINE_LEVELS = L.N_LEVELS, L.N_LINE_LEVELS
SCALE_FACTORS, LINE_SCALE_FACTORS, LINE_INV_SIGMA2 = L.SCALE_FACTORS, L.LINE_SCALE_FACTORS, L.LINE_INV_SIGMA2
SPECIAL = np.array([0.4, -0.3, 0.2], f32)
N_KP, N_KL = 200, 40
DIRECTIONS = ("neither", "forward", "backward")
SEARCH_CASES = [(th, check, occ, d) for th in (7.0, 15.0) for check in (1, 0) for occ in (1, 0) for d in DIRECTIONS]
NN_RATIO_LINES = 0.9


def _quat():
    a = np.array([1.0, 2.0, 0.5])
    a /= np.linalg.norm(a)
    q = np.concatenate([np.sin(0.125) * a, [np.cos(0.125)]])
    return q.astype(f32)


def _rot64(q):
    x, y, z, w = (float(c) for c in q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def poses(direction="neither", mono=0):
    """The current pose and one of three last-frame poses: tlc(2) = +0.5 / -0.5 / 0.01 against mb = 0.08."""
    q = _quat()
    Rm = _rot64(q)
    with np.errstate(all="ignore"):
        tcw = (-R.se3_act(q, np.zeros(3, f32), SPECIAL)[0]).astype(f32)          # q * special + tcw == 0 exactly, in all three
    Rcw = np.ascontiguousarray(Rm.astype(f32).T.reshape(-1))                    # column-major, as mRcw lies in memory
    Ow = (-(Rm.T @ tcw.astype(np.float64))).astype(f32)
    dz = dict(neither=0.01, forward=0.5, backward=-0.5)[direction]
    tlw = (tcw.astype(np.float64) + np.array([0.02, -0.01, dz])).astype(f32)
    return dict(q_cw=q, tcw=tcw, Rcw=Rcw, Ow=Ow, q_lw=q.copy(), tlw=tlw, mb=MB, mbf=MBF, bounds4=BOUNDS4, K4=K4, K4_linear=None, mono=mono)


def _world(P, u, v, z):
    """World points (f32) that project near (u, v) at camera depth z."""
    Rm = _rot64(P["q_cw"])
    u, v, z = np.atleast_1d(np.asarray(u, np.float64)), np.atleast_1d(np.asarray(v, np.float64)), np.asarray(z, np.float64)
    xc = np.stack([(u - float(K4[2])) * z / float(K4[0]), (v - float(K4[3])) * z / float(K4[1]), z * np.ones_like(u)], -1)
    return ((xc - P["tcw"].astype(np.float64)) @ Rm).astype(f32)


def _ulp_grid(p, span):
    """p [3] with its first two coordinates moved by -span .. span ulps: [(2 span + 1)^2, 3]."""
    xs, ys = [p[0]], [p[1]]
    for _ in range(span):
        xs = [np.nextafter(xs[0], f32(-np.inf))] + xs + [np.nextafter(xs[-1], f32(np.inf))]
        ys = [np.nextafter(ys[0], f32(-np.inf))] + ys + [np.nextafter(ys[-1], f32(np.inf))]
    g = np.array([(x, y, p[2]) for x in xs for y in ys], f32)
    return g


def _on_bound(P, u, v, z, want_u=None, want_v=None):
    """A world point near (u, v, z) whose projection has u == want_u or v == want_v EXACTLY in the reference's f32 sequence."""
    p = _world(P, u, v, z)[0]
    g = _ulp_grid(p, 40)
    r = R.project_points(P, dict(valid=np.ones(len(g), np.uint8), pos=g))
    hit = (r["u"] == f32(want_u)) if want_u is not None else (r["v"] == f32(want_v))
    assert hit.any(), "no float on the bound within 40 ulps"
    return g[np.flatnonzero(hit)[0]]


def _plus_zero_inf(P):
    """A world point other than `special` with x3Dc(2) == +0.0f exactly and x3Dc(0) != 0."""
    Rm = _rot64(P["q_cw"])
    p = (SPECIAL.astype(np.float64) + Rm.T @ np.array([0.25, 0.1, 0.0])).astype(f32)
    g = _ulp_grid(np.array([p[2], p[1], p[0]], f32), 60)[:, ::-1]          # move z and y
    with np.errstate(all="ignore"):
        pc = R.se3_act(P["q_cw"], P["tcw"], g)
    hit = (pc[:, 2] == 0) & (pc[:, 0] != 0)
    assert hit.any(), "no float with a zero depth within 60 ulps"
    return np.ascontiguousarray(g[np.flatnonzero(hit)[0]])


def _max_on_edge(dist, factor):
    """mfMaxDistance (f32) with f32(factor * max) == dist exactly, and its neighbour on the rejecting side."""
    c = f32(dist / factor)
    for k in range(-8, 9):
        m = L._ulps(c, k)
        if f32(factor) * m == dist:
            step = 1 if factor < 1 else -1          # 0.8f * max > dist rejects (too near); 1.2f * max < dist rejects (too far)
            o = m
            while (f32(factor) * o == dist):
                o = L._ulps(o, step)
            return m, o
    return None, None


def inputs(direction="neither", mono=0):
    rng = np.random.default_rng(SEED)
    P = poses(direction, mono)
    fr = L._frame(rng, N_KP, N_KL)
    cur_angle = rng.uniform(0, 360, N_KP).astype(f32)
    where = {}
    pts = dict(valid=[], pos=[], octave=[], angle=[], desc=[])

    def add(pos, octave, angle, desc, valid=1):
        pts["valid"].append(valid); pts["pos"].append(np.asarray(pos, f32)); pts["octave"].append(int(octave))
        pts["angle"].append(f32(angle)); pts["desc"].append(desc)
        return len(pts["valid"]) - 1

    rnd = lambda: rng.integers(0, 256, 32, dtype=np.uint8)

    def matching(i, du=0.0, dv=0.0, octave=None, wild=False):
        p = _world(P, fr["x"][i] + du, fr["y"][i] + dv, fr["depth"][i])[0]
        ang = rng.uniform(0, 360) if wild else (cur_angle[i] + 20 + rng.normal(0, 4)) % 360
        return add(p, fr["octave"][i] if octave is None else octave, ang, L._flip(rng, fr["desc"][i], int(rng.integers(0, 24))))

    order = [int(i) for i in rng.permutation(N_KP)]
    oct0 = [i for i in order if fr["octave"][i] == 0]
    top = [i for i in order if fr["octave"][i] == N_LEVELS - 1]
    # accepted at octave 0 and at the top octave, with (even key points) and without u_right
    corner = [next(i for i in oct0 if i % 2 == 0), next(i for i in oct0 if i % 2 == 1), next(i for i in top if i % 2 == 0),
              next(i for i in top if i % 2 == 1)]
    where["octave_0"] = [matching(corner[0]), matching(corner[1])]
    where["octave_top"] = [matching(corner[2]), matching(corner[3])]
    rest = [i for i in order if i not in corner]
    where["match"] = [matching(i, du=rng.normal(0, 1.5), dv=rng.normal(0, 1.5), octave=int(np.clip(fr["octave"][i] + rng.integers(-1, 2), 0, N_LEVELS - 1)),
                               wild=rng.random() < 0.15) for i in rest[:52]]
    low = [i for i in rest[52:] if fr["octave"][i] <= 2 and 90 < fr["x"][i] < W - 90]
    where["wide"] = [matching(i, du=1.5 * 15.0 * float(SCALE_FACTORS[fr["octave"][i]]) * (1 if k % 2 else -1)) for k, i in enumerate(low[:18])]
    where["mid"] = [matching(i, du=11.0 * float(SCALE_FACTORS[fr["octave"][i]]) * (1 if k % 2 else -1)) for k, i in enumerate(low[18:26])]
    where["invalid"] = [add(_world(P, rng.uniform(50, 590), rng.uniform(50, 430), rng.uniform(1, 5))[0], rng.integers(0, 8), 0.0, rnd(), valid=0)
                        for _ in range(4)]
    free = lambda u, v, z: add(_world(P, u, v, z)[0], rng.integers(0, N_LEVELS), rng.uniform(0, 360), rnd())
    where["behind"] = [free(rng.uniform(100, 500), rng.uniform(100, 400), -rng.uniform(0.5, 4.0)) for _ in range(4)]
    where["out_left"] = [free(-rng.uniform(5, 200), rng.uniform(50, 430), rng.uniform(1, 5)) for _ in range(2)]
    where["out_right"] = [free(W + rng.uniform(5, 200), rng.uniform(50, 430), rng.uniform(1, 5)) for _ in range(2)]
    where["out_top"] = [free(rng.uniform(50, 590), -rng.uniform(5, 200), rng.uniform(1, 5)) for _ in range(2)]
    where["out_bottom"] = [free(rng.uniform(50, 590), H + rng.uniform(5, 200), rng.uniform(1, 5)) for _ in range(2)]
    on = lambda p: add(p, rng.integers(0, N_LEVELS), rng.uniform(0, 360), rnd())
    where["on_left"] = [on(_on_bound(P, 0.0, 200.0, 2.0, want_u=0.0))]
    where["on_right"] = [on(_on_bound(P, float(W), 260.0, 3.0, want_u=float(W)))]
    where["on_top"] = [on(_on_bound(P, 300.0, 0.0, 2.5, want_v=0.0))]
    where["on_bottom"] = [on(_on_bound(P, 340.0, float(H), 3.5, want_v=float(H)))]
    where["z_plus_zero_nan"] = [add(SPECIAL, 3, 10.0, rnd())]
    where["z_plus_zero_inf"] = [add(_plus_zero_inf(P), 3, 10.0, rnd())]
    n = len(pts["valid"])
    points = dict(valid=np.array(pts["valid"], np.uint8), pos=np.array(pts["pos"], f32).reshape(n, 3), octave=np.array(pts["octave"], np.int32),
                  angle=np.array(pts["angle"], f32), desc=np.array(pts["desc"], np.uint8).reshape(n, 32), has_obs=(rng.random(n) < 0.95).astype(np.uint8))

    # ---- last-frame lines
    kl = fr["keylines"]
    Ls = dict(valid=[], start=[], end=[], max_dist=[], octave=[], angle=[], desc=[])

    def dist_of(s, e):
        return R.project_lines(P, dict(valid=np.ones(1, np.uint8), start=s[None], end=e[None], max_dist=np.ones(1, f32)))["dist"][0]

    def add_line(s, e, max_of, octave, angle, desc, valid=1):
        s, e = np.asarray(s, f32), np.asarray(e, f32)
        Ls["valid"].append(valid); Ls["start"].append(s); Ls["end"].append(e); Ls["max_dist"].append(f32(max_of(dist_of(s, e))))
        Ls["octave"].append(int(octave)); Ls["angle"].append(f32(angle)); Ls["desc"].append(desc)
        return len(Ls["valid"]) - 1

    def line_of(j, zs=None, ze=None, shift=0.0, us=None, ue=None):
        zs = fr["line_depth"][j, 0] if zs is None else zs
        ze = fr["line_depth"][j, 1] if ze is None else ze
        xs, ys, xe, ye = (float(kl[k][j]) for k in ("startPointX", "startPointY", "endPointX", "endPointY"))
        nx, ny = ye - ys, xs - xe
        nn = np.hypot(nx, ny)
        xs, ys, xe, ye = xs + shift * nx / nn, ys + shift * ny / nn, xe + shift * nx / nn, ye + shift * ny / nn
        xs, xe = (xs if us is None else us), (xe if ue is None else ue)
        return _world(P, xs, ys, zs)[0], _world(P, xe, ye, ze)[0]

    def matching_line(j, shift=0.0, octave=None, turn=0.0):
        s, e = line_of(j, shift=shift)
        return add_line(s, e, lambda d: d * rng.uniform(0.9, 1.1), int(kl["octave"][j]) if octave is None else octave,
                        float(kl["angle"][j]) + 0.04 + rng.normal(0, 0.02) + turn, L._flip(rng, fr["line_desc"][j], int(rng.integers(0, 24))))

    lorder = [int(j) for j in rng.permutation(N_KL)]
    # every fourth one level above / below its key line (the bands of bForward / bBackward), four with a turned angle each in a bin of its own (the histogram keeps three bins)
    where["line_match"] = [matching_line(j, octave=int(np.clip(int(kl["octave"][j]) + {1: 1, 2: -1}.get(k % 4, 0), 0, N_LINE_LEVELS - 1)),
                                         turn={3: 2.0, 6: 1.0, 9: 4.0, 11: 3.0}.get(k, 0.0)) for k, j in enumerate(lorder[:14])]
    where["line_shifted"] = [matching_line(j, shift=2.1, octave=0) for j in lorder[14:20]]
    lfree = lorder[20:]
    plain = lambda s, e, max_of=lambda d: d, valid=1: add_line(s, e, max_of, rng.integers(0, N_LINE_LEVELS), rng.uniform(-3, 3), rnd(), valid)
    where["line_invalid"] = [plain(*line_of(lfree[0]), valid=0), plain(*line_of(lfree[1]), valid=0)]
    where["line_middle_behind"] = [plain(*line_of(lfree[2], zs=-2.0, ze=-3.0))]

    def seg(u, v, du=20.0, dv=20.0, zs=3.0, ze=3.2):
        return _world(P, u, v, zs)[0], _world(P, u + du, v + dv, ze)[0]

    where["line_middle_out"] = [plain(*seg(-150.0, 200.0)), plain(*seg(W + 150.0, 200.0)), plain(*seg(300.0, -150.0)), plain(*seg(300.0, H + 150.0))]
    where["line_too_near"] = [plain(*line_of(lfree[3]), max_of=lambda d: d * 1.4)]          # 0.8f * max = 1.12 d > d
    where["line_too_far"] = [plain(*line_of(lfree[4]), max_of=lambda d: d * 0.8)]           # 1.2f * max = 0.96 d < d
    k = 5
    for name, factor in (("near", 0.8), ("far", 1.2)):
        m = None
        while m is None:
            s, e = line_of(lfree[k])
            k += 1
            m, o = _max_on_edge(dist_of(s, e), factor)
        where[f"line_on_{name}_edge"] = [plain(s, e, max_of=lambda d, m=m: m)]
        where[f"line_past_{name}_edge"] = [plain(s, e, max_of=lambda d, o=o: o)]
    where["line_start_behind"] = [plain(*seg(250.0, 200.0, 80.0, 40.0, zs=-0.5, ze=4.0))]
    where["line_end_behind"] = [plain(*seg(250.0, 260.0, 80.0, 40.0, zs=4.0, ze=-0.5))]
    where["line_start_out"] = [plain(*seg(-60.0, 220.0, 400.0, 30.0))]
    where["line_end_out"] = [plain(*seg(300.0, 220.0, 400.0, 30.0))]
    nl = len(Ls["valid"])
    lines = dict(valid=np.array(Ls["valid"], np.uint8), start=np.array(Ls["start"], f32).reshape(nl, 3), end=np.array(Ls["end"], f32).reshape(nl, 3),
                 max_dist=np.array(Ls["max_dist"], f32), octave=np.array(Ls["octave"], np.int32), angle=np.array(Ls["angle"], f32),
                 desc=np.array(Ls["desc"], np.uint8).reshape(nl, 32), has_obs=(rng.random(nl) < 0.9).astype(np.uint8))
    frame = dict(x=fr["x"], y=fr["y"], octave=fr["octave"], u_right=fr["u_right"], desc=fr["desc"], cur_angle=cur_angle, keylines=kl,
                 line_desc=fr["line_desc"], u_right_start=fr["u_right_start"], u_right_end=fr["u_right_end"],
                 occupied_points=(rng.random(N_KP) < 0.08).astype(np.uint8), occupied_lines=(rng.random(N_KL) < 0.08).astype(np.uint8))
    return dict(poses=P, frame=frame, points=points, lines=lines, where=where)


def policy_inputs(kind):
    """The base set with the valid flags cut so that the retry rules of Tracking.cc:3626-3663 run (see the module's text)."""
    inp = inputs()
    w = inp["where"]
    points, lines = dict(inp["points"]), dict(inp["lines"])
    if kind == "few_points":
        keep = set(w["match"][:12]) | set(w["wide"])
        points["valid"] = np.array([1 if i in keep else 0 for i in range(len(points["valid"]))], np.uint8)
    elif kind == "few_lines":
        keep = set(w["line_match"][:6]) | set(w["line_shifted"])
        lines["valid"] = np.array([1 if i in keep else 0 for i in range(len(lines["valid"]))], np.uint8)
    else:
        assert kind == "plain"
    out = dict(inp)
    out["points"], out["lines"] = points, lines
    return out


POLICY_KINDS = ("plain", "few_points", "few_lines")


def crowd_inputs():
    """200 last-frame points at the top octave over one cluster of 300 key points: every window holds the whole cluster, 60 000
    candidates against a first capacity of 200 * 32 + 4096."""
    rng = np.random.default_rng(SEED + 1)
    P = poses()
    n, m = 300, 200
    x, y = (320 + rng.uniform(-6, 6, n)).astype(f32), (240 + rng.uniform(-6, 6, n)).astype(f32)
    octave = rng.integers(6, 8, n).astype(np.int32)
    base = rng.integers(0, 256, 32, dtype=np.uint8)
    desc = np.array([L._flip(rng, base, int(rng.integers(0, 60))) for _ in range(n)], np.uint8)
    depth = rng.uniform(2.0, 4.0, n)
    u_right = np.where(np.arange(n) % 3 == 0, x - float(MBF) / depth, -1).astype(f32)
    src = rng.integers(0, n, m)
    cur_angle = rng.uniform(0, 360, n).astype(f32)
    points = dict(valid=np.ones(m, np.uint8), pos=_world(P, x[src], y[src], depth[src]), octave=np.full(m, 7, np.int32),
                  angle=((cur_angle[src] + 20 + rng.normal(0, 4, m)) % 360).astype(f32),
                  desc=np.array([L._flip(rng, desc[i], int(rng.integers(0, 20))) for i in src], np.uint8), has_obs=(rng.random(m) < 0.95).astype(np.uint8))
    frame = dict(x=x, y=y, octave=octave, u_right=u_right, desc=desc, cur_angle=cur_angle, occupied_points=(rng.random(n) < 0.05).astype(np.uint8))
    return dict(poses=P, frame=frame, points=points, lines=None, where={})


def minus_zero_inputs():
    """A pose and a point with x3Dc(2) == -0.0f in the reference's f32 sequence (invzc = -inf < 0: rejected before the projection),
    the same point with z == +0.0f (invzc = +inf, u = -inf: rejected by the bounds), a point behind the camera, an invalid one, and
    eight points the half turn accepts, over 12 key points.  No lines."""
    rng = np.random.default_rng(SEED + 2)
    q = np.array([0.0, 1e-30, -1.0, 0.0], f32)                                  # |q| == 1 in f32 and in f64
    tcw = np.array([0.0, 0.0, -0.0], f32)
    P = dict(q_cw=q, tcw=tcw, Rcw=np.ascontiguousarray(_rot64(q).astype(f32).T.reshape(-1)), Ow=np.zeros(3, f32), q_lw=q.copy(),
             tlw=np.array([0.02, -0.01, 0.01], f32), mb=MB, mbf=MBF, bounds4=BOUNDS4, K4=K4, K4_linear=None, mono=0)
    n, m = 12, 8
    x, y = rng.uniform(100, 540, n).astype(f32), rng.uniform(100, 380, n).astype(f32)
    octave = rng.integers(0, N_LEVELS, n).astype(np.int32)
    desc = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    depth = rng.uniform(2.0, 4.0, n)
    u_right = np.where(np.arange(n) % 3 == 0, x - float(MBF) / depth, -1).astype(f32)
    cur_angle = rng.uniform(0, 360, n).astype(f32)
    src = rng.permutation(n)[:m]
    pos = [p for p in _world(P, x[src] + rng.normal(0, 1.0, m), y[src] + rng.normal(0, 1.0, m), depth[src])]
    where = dict(match=list(range(m)), z_minus_zero=[m], z_plus_zero=[m + 1], behind=[m + 2], invalid=[m + 3])
    pos += [np.array([1.0, 0.0, -0.0], f32), np.array([1.0, 0.0, 0.0], f32), _world(P, 300.0, 200.0, -2.0)[0], _world(P, 300.0, 200.0, 2.0)[0]]
    k = len(pos)
    extra = k - m
    points = dict(valid=np.array([1] * (k - 1) + [0], np.uint8), pos=np.array(pos, f32).reshape(k, 3),
                  octave=np.concatenate([octave[src], rng.integers(0, N_LEVELS, extra)]).astype(np.int32),
                  angle=np.concatenate([(cur_angle[src] + 20 + rng.normal(0, 4, m)) % 360, rng.uniform(0, 360, extra)]).astype(f32),
                  desc=np.array([L._flip(rng, desc[i], int(rng.integers(0, 20))) for i in src] + [rng.integers(0, 256, 32, dtype=np.uint8) for _ in range(extra)],
                                np.uint8).reshape(k, 32), has_obs=np.ones(k, np.uint8))
    frame = dict(x=x, y=y, octave=octave, u_right=u_right, desc=desc, cur_angle=cur_angle, occupied_points=np.zeros(n, np.uint8))
    return dict(poses=P, frame=frame, points=points, lines=None, where=where)


def random_inputs(n=1500, nl=300, seed=5, n_kp=1500, n_kl=300):
    """The timing set, and with other sizes the size tests': last-frame points / lines around the frustum of a frame of n_kp key
    points and n_kl key lines."""
    rng = np.random.default_rng(seed)
    P = poses()
    fr = L._frame(rng, n_kp, n_kl)
    kl = fr["keylines"]
    cur_angle = rng.uniform(0, 360, n_kp).astype(f32)
    src = rng.integers(0, n_kp, n)
    jit = rng.normal(0, 2.0, (n, 2))
    out = rng.random(n) < 0.2
    jit[out] += rng.normal(0, 400, (int(out.sum()), 2))
    pos = _world(P, fr["x"][src] + jit[:, 0], fr["y"][src] + jit[:, 1], fr["depth"][src] * np.where(rng.random(n) < 0.05, -1, 1)).reshape(n, 3)
    pdesc = fr["desc"][src] ^ (rng.integers(0, 256, (n, 32), dtype=np.uint8) & rng.integers(0, 256, (n, 32), dtype=np.uint8)
                               & rng.integers(0, 256, (n, 32), dtype=np.uint8) & rng.integers(0, 256, (n, 32), dtype=np.uint8))
    points = dict(valid=(rng.random(n) < 0.9).astype(np.uint8), pos=pos, octave=np.clip(fr["octave"][src] + rng.integers(-1, 2, n), 0, N_LEVELS - 1).astype(np.int32),
                  angle=((cur_angle[src] + 20 + rng.normal(0, 5, n)) % 360).astype(f32), desc=pdesc, has_obs=(rng.random(n) < 0.95).astype(np.uint8))
    lsrc = rng.integers(0, n_kl, nl)
    zs = fr["line_depth"][lsrc, 0] * np.where(rng.random(nl) < 0.05, -1, 1)
    ze = fr["line_depth"][lsrc, 1]
    start = _world(P, kl["startPointX"][lsrc].astype(np.float64) + rng.normal(0, 0.5, nl), kl["startPointY"][lsrc].astype(np.float64), zs).reshape(nl, 3)
    end = _world(P, kl["endPointX"][lsrc].astype(np.float64) + rng.normal(0, 0.5, nl), kl["endPointY"][lsrc].astype(np.float64), ze).reshape(nl, 3)
    lines = dict(valid=(rng.random(nl) < 0.9).astype(np.uint8), start=start, end=end, max_dist=np.ones(nl, f32), octave=kl["octave"][lsrc].astype(np.int32),
                 angle=(kl["angle"][lsrc] + 0.04 + rng.normal(0, 0.03, nl)).astype(f32),
                 desc=fr["line_desc"][lsrc] ^ (rng.integers(0, 256, (nl, 32), dtype=np.uint8) & rng.integers(0, 256, (nl, 32), dtype=np.uint8)
                                               & rng.integers(0, 256, (nl, 32), dtype=np.uint8)), has_obs=(rng.random(nl) < 0.9).astype(np.uint8))
    if nl:
        d = R.project_lines(P, lines)["dist"].astype(np.float64)
        lines["max_dist"] = (d * rng.uniform(0.75, 1.3, nl)).astype(f32)
    frame = dict(x=fr["x"], y=fr["y"], octave=fr["octave"], u_right=fr["u_right"], desc=fr["desc"], cur_angle=cur_angle, keylines=kl,
                 line_desc=fr["line_desc"], u_right_start=fr["u_right_start"], u_right_end=fr["u_right_end"],
                 occupied_points=(rng.random(n_kp) < 0.08).astype(np.uint8), occupied_lines=(rng.random(n_kl) < 0.08).astype(np.uint8))
    return dict(poses=P, frame=frame, points=points, lines=lines, where={})


def inputs_digest(inp):
    h = hashlib.sha1()
    P = inp["poses"]
    for k in ("q_cw", "tcw", "Rcw", "Ow", "q_lw", "tlw", "bounds4", "K4"):
        h.update(np.ascontiguousarray(P[k], f32).tobytes())
    h.update(np.array([P["mb"], P["mbf"]], f32).tobytes())
    for part in ("frame", "points", "lines"):
        if inp[part] is not None:
            for k in sorted(inp[part]):
                h.update(np.ascontiguousarray(inp[part][k]).tobytes())
    return h.hexdigest()


def frame_view(inp):
    """orbmatcher.FrameView of a set's frame."""
    from plvs_amd.orbmatcher import FrameView
    fr = inp["frame"]
    return FrameView(fr["x"], fr["y"], fr["octave"], fr["u_right"], fr["desc"], 0.0, 0.0, L.GRID_W_INV, L.GRID_H_INV, SCALE_FACTORS)


def line_view(inp):
    """linematcher.line_frame_view of a set's frame (None without lines)."""
    from plvs_amd.linematcher import line_frame_view
    fr = inp["frame"]
    if "keylines" not in fr:
        return None
    return line_frame_view(fr["keylines"], fr["line_desc"], LINE_SCALE_FACTORS, LINE_INV_SIGMA2, L.MAX_DIAG, fr["u_right_start"], fr["u_right_end"],
                           float(MBF))


def search_key(th, check, occ, direction):
    return f"assigned_points_th{int(th)}_check{int(check)}_occ{int(occ)}_{direction}"


def line_key(check, occ, direction, larger=0):
    return f"assigned_lines_larger{int(larger)}_check{int(check)}_occ{int(occ)}_{direction}"


# ---- the search stage behind the projection, by the oracle's restatement that tests/test_oracle_pinned_matchers.py pins to the
# compiled reference (oracle_orb_search_by_projection_ff / oracle_lines_search_by_projection_ff): it accepts the projected fields
def _p(a):
    import ctypes
    return None if a is None else np.ascontiguousarray(a).ctypes.data_as(ctypes.c_void_p)


def direction_code(forward, backward):
    return 1 if forward else (2 if backward else 0)


def oracle_point_search(olib, inp, fields, th, forward, backward, check, occ):
    """fields: dict(proj_valid, u, v, invz) -> (nmatches, assigned [N])."""
    import ctypes
    from plvs_amd.orbmatcher import LastFrameView
    vp, i, fl = ctypes.c_void_p, ctypes.c_int, ctypes.c_float
    pts, fr = inp["points"], inp["frame"]
    fv = frame_view(inp)
    lf = LastFrameView(valid=fields["proj_valid"], u=fields["u"], v=fields["v"], invz=fields["invz"], octave=pts["octave"], angle=pts["angle"],
                       desc=pts["desc"], has_obs=pts.get("has_obs"))
    fc, lc = fv.as_c(), lf.as_c()
    a = np.full(max(fc.n, 1), -7, np.int32)
    fn = olib.oracle_orb_search_by_projection_ff
    fn.restype = i
    fn.argtypes = [vp, vp, fl, fl, fl, vp, fl, i, i, i, vp, vp]
    n = fn(ctypes.byref(fc), _p(fr["cur_angle"]), float(BOUNDS4[1]), float(BOUNDS4[3]), float(MBF), ctypes.byref(lc), float(th), int(forward),
           int(backward), int(check), _p(fr["occupied_points"]) if occ else None, _p(a))
    return n, a[:fc.n]


def oracle_line_search(olib, inp, fields, larger, direction, check, occ, nn_ratio=NN_RATIO_LINES):
    """fields: dict(proj_valid, proj6); direction: 0, 1 forward, 2 backward -> (nmatches, assigned [Nlines])."""
    import ctypes
    vp, i, fl = ctypes.c_void_p, ctypes.c_int, ctypes.c_float
    ln, fr = inp["lines"], inp["frame"]
    kl = np.ascontiguousarray(fr["keylines"])
    a = np.full(max(len(kl), 1), -7, np.int32)
    fn = olib.oracle_lines_search_by_projection_ff
    fn.restype = i
    fn.argtypes = [i, vp, vp, vp, vp, fl, vp, vp, fl, vp, i, vp, vp, vp, vp, vp, vp, i, i, fl, i, vp]
    n = fn(len(kl), _p(kl), _p(fr["line_desc"]), _p(fr["u_right_start"]), _p(fr["u_right_end"]), float(MBF), _p(LINE_SCALE_FACTORS),
           _p(LINE_INV_SIGMA2), float(L.MAX_DIAG), _p(fr["occupied_lines"]) if occ else None, len(ln["valid"]), _p(fields["proj_valid"]),
           _p(np.asarray(fields["proj6"], f32)), _p(ln["octave"]), _p(ln["angle"]), _p(ln["desc"]), _p(ln.get("has_obs")), int(larger),
           int(direction), float(nn_ratio), int(check), _p(a))
    return n, a[:len(kl)]
