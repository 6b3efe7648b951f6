"""ORBmatcher::SearchByProjection(Frame, MapPoints) (reference src/ORBmatcher.cc:71-244): the
oracle restatement (oracle/orb_search.c) and the library function built on the batched
candidate-pair Hamming kernel must give identical assignments."""
import ctypes

import numpy as np
import pytest

from tests import oracle_lib


def make_case(seed, n=1500, m=900, w=640, h=480, occupied_frac=0.1):
    """A frame of n keypoints and m map points that mostly re-observe them."""
    from plvs_amd.orbmatcher import FrameView, MapPointView
    rng = np.random.default_rng(seed)
    scale = (1.2 ** np.arange(8)).astype(np.float32)
    x = rng.uniform(0, w, n).astype(np.float32)
    y = rng.uniform(0, h, n).astype(np.float32)
    octave = rng.integers(0, 8, n).astype(np.int32)
    desc = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    u_right = np.where(rng.random(n) < 0.7, x - rng.uniform(2, 40, n), -1).astype(np.float32)
    F = FrameView(x, y, octave, u_right, desc, 0.0, 0.0, 64.0 / w, 48.0 / h, scale)
    src = rng.integers(0, n, m)
    noise = rng.normal(0, 3.0, (m, 2)).astype(np.float32)
    mdesc = desc[src].copy()
    flips = rng.integers(0, 256, (m, 32), dtype=np.uint8) & rng.integers(0, 256, (m, 32), dtype=np.uint8) \
        & rng.integers(0, 256, (m, 32), dtype=np.uint8) & rng.integers(0, 256, (m, 32), dtype=np.uint8)
    mdesc ^= flips                                   # ~16 flipped bits: distances around the thresholds
    rnd = rng.random(m) < 0.15                        # some map points that match nothing
    mdesc[rnd] = rng.integers(0, 256, (int(rnd.sum()), 32), dtype=np.uint8)
    level = np.clip(octave[src] + rng.integers(-1, 2, m), 0, 7).astype(np.int32)
    M = MapPointView(track_in_view=(rng.random(m) < 0.9), bad=(rng.random(m) < 0.03),
                     proj_x=x[src] + noise[:, 0], proj_y=y[src] + noise[:, 1],
                     proj_xr=np.where(u_right[src] > 0, u_right[src] + rng.normal(0, 2.0, m), -1),
                     view_cos=rng.uniform(0.99, 1.0, m), track_depth=rng.uniform(0.5, 60.0, m), level=level,
                     desc=mdesc, has_obs=(rng.random(m) < 0.97))
    occupied = (rng.random(n) < occupied_frac).astype(np.uint8)
    return F, M, occupied


def oracle_search(lib, F, M, th, far, th_far, ratio, occupied):
    fc, mc = F.as_c(), M.as_c()
    assigned = np.full(fc.n, -7, np.int32)
    f = lib.oracle_orb_search_by_projection
    f.restype = ctypes.c_int
    f.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_float, ctypes.c_int, ctypes.c_float, ctypes.c_float,
                  ctypes.c_void_p, ctypes.c_void_p]
    n = f(ctypes.byref(fc), ctypes.byref(mc), th, int(far), th_far, ratio,
          occupied.ctypes.data_as(ctypes.c_void_p), assigned.ctypes.data_as(ctypes.c_void_p))
    return n, assigned


def test_oracle_search_by_projection_properties(oracle):
    """Known answers on a hand-made frame + invariants on a random one."""
    from plvs_amd.orbmatcher import FrameView, MapPointView
    lib = oracle.lib
    scale = (1.2 ** np.arange(8)).astype(np.float32)
    d = np.zeros((3, 32), np.uint8)
    d[1, 0] = 0xFF            # keypoint 1: 8 bits from keypoint 0
    d[2, :13] = 0xFF          # keypoint 2: 104 bits away: above TH_HIGH
    F = FrameView(np.array([100, 101.5, 300], np.float32), np.array([100, 100, 300], np.float32),
                  np.array([2, 2, 2], np.int32), np.array([-1, -1, -1], np.float32), d, 0, 0, 0.1, 0.1, scale)
    one = lambda v, t=np.float32: np.array([v], t)
    M = MapPointView(one(1, np.uint8), one(0, np.uint8), one(100.2), one(100.1), one(-1), one(0.9999), one(3.0),
                     one(2, np.int32), d[:1].copy())
    # best = kp 0 (distance 0), second = kp 1 (distance 8) on the same level: 0 <= ratio * 8 -> matched
    n, a = oracle_search(lib, F, M, 1.0, False, 0.0, 0.8, np.zeros(3, np.uint8))
    assert n == 1 and list(a) == [0, -1, -1]
    # keypoint 0 occupied: the best free candidate is kp 1 (8 <= 100), no second -> bestLevel2 = -1 != 2 -> matched
    n, a = oracle_search(lib, F, M, 1.0, False, 0.0, 0.8, np.array([1, 0, 0], np.uint8))
    assert n == 1 and list(a) == [-1, 0, -1]
    # a far point is skipped when bFarPoints is set
    n, a = oracle_search(lib, F, M, 1.0, True, 2.0, 0.8, np.zeros(3, np.uint8))
    assert n == 0 and list(a) == [-1, -1, -1]
    # random case: every assignment respects the window, the level band, TH_HIGH and uniqueness
    F, M, occ = make_case(3)
    n, a = oracle_search(lib, F, M, 1.0, False, 0.0, 0.8, occ)
    got = np.nonzero(a >= 0)[0]
    # (a map point without observations does not block its keypoint: a later one may take it over,
    # and the reference counts both)
    assert n >= len(got) > 100 and n - len(got) <= int((~M.has_obs.astype(bool)).sum())
    assert not occ[got].any()
    for i in got:
        k = a[i]
        r = (2.5 if M.view_cos[k] > 0.998 else 4.0) * F.scale_factors[M.level[k]]
        assert abs(F.x[i] - M.proj_x[k]) < r and abs(F.y[i] - M.proj_y[k]) < r
        assert M.level[k] - 1 <= F.octave[i] <= M.level[k]
        assert oracle.descriptor_distance(M.desc[k], F.desc[i]) <= 100
        assert M.track_in_view[k] and not M.bad[k]


@pytest.mark.gpu
@pytest.mark.parametrize("seed,th,far", [(1, 1.0, False), (2, 3.0, False), (5, 1.0, True), (8, 5.0, True)])
def test_hip_search_by_projection_matches_oracle(oracle, seed, th, far):
    from plvs_amd.orbmatcher import ORBmatcher
    F, M, occ = make_case(seed)
    want_n, want = oracle_search(oracle.lib, F, M, th, far, 40.0, 0.8, occ)
    got_n, got = ORBmatcher(0.8, True).SearchByProjection(F, M, th, far, 40.0, occupied=occ)
    assert got_n == want_n > 50
    assert np.array_equal(got, want)


@pytest.mark.gpu
def test_hip_hamming_pairs_and_edge_cases(oracle):
    from plvs_amd import _lib
    from plvs_amd.orbmatcher import FrameView, MapPointView, ORBmatcher
    rng = np.random.default_rng(0)
    q = rng.integers(0, 256, (50, 32), dtype=np.uint8)
    t = rng.integers(0, 256, (70, 32), dtype=np.uint8)
    pq = rng.integers(0, 50, 4000).astype(np.int32)
    pt = rng.integers(0, 70, 4000).astype(np.int32)
    d = np.zeros(4000, np.int32)
    _lib.check(_lib.lib.plvs_hip_hamming_pairs(_lib.np_ptr(q), 50, _lib.np_ptr(t), 70, _lib.np_ptr(pq), _lib.np_ptr(pt),
                                               4000, _lib.np_ptr(d)))
    ref = np.unpackbits(q[pq] ^ t[pt], axis=1).sum(1)
    assert np.array_equal(d, ref)
    assert ORBmatcher.DescriptorDistance(q[3], t[9]) == oracle.descriptor_distance(q[3], t[9])
    # empty inputs: nothing assigned, zero matches
    F, M, occ = make_case(4, n=40, m=0)
    n, a = ORBmatcher(0.8).SearchByProjection(F, M, occupied=occ)
    assert n == 0 and (a == -1).all()
    # out-of-range pair index is an error, not a fault
    bad = np.array([999], np.int32)
    rc = _lib.lib.plvs_hip_hamming_pairs(_lib.np_ptr(q), 50, _lib.np_ptr(t), 70, _lib.np_ptr(bad), _lib.np_ptr(bad), 1,
                                         _lib.np_ptr(d))
    assert rc != 0


# ------------------------------------------------------------------ crowds, borders, the spill path
CROWD_W, CROWD_H = 640, 480
CROWD_MIN_X, CROWD_MIN_Y = -12.5, -7.25                      # undistorted bounds reach outside the image
CROWD_MAX_X, CROWD_MAX_Y = CROWD_W + 12.5, CROWD_H + 7.25


def _flip16(rng, desc):
    """Copies with ~16 flipped bits (four ANDed random bytes leave a bit set with probability 1/16)."""
    m = desc.shape[0]
    f = rng.integers(0, 256, (m, 32), dtype=np.uint8)
    for _ in range(3):
        f &= rng.integers(0, 256, (m, 32), dtype=np.uint8)
    return desc ^ f


def make_crowd_frame(seed, n_crowd=256):
    """A frame whose grid has non-zero origin: n_crowd keypoints within +-4 px of (300, 200) (one or two cells, one
    column range of > 250 members), 32 on the min / max borders, 32 whose PosInGrid column is 64 (outside the grid).
    -> (FrameView, dict of the index sets after the shuffle)."""
    from plvs_amd.orbmatcher import FrameView
    rng = np.random.default_rng(seed)
    scale = (1.2 ** np.arange(8)).astype(np.float32)
    cx, cy = 300 + rng.uniform(-4, 4, n_crowd), 200 + rng.uniform(-4, 4, n_crowd)
    lo, hi = rng.uniform(0.05, 0.55, 32), rng.uniform(5.5, 6.0, 32)
    bx = np.concatenate([CROWD_MIN_X + lo[:8], CROWD_MAX_X - hi[8:16], rng.uniform(20, CROWD_W - 20, 16)])
    by = np.concatenate([rng.uniform(20, CROWD_H - 20, 16), CROWD_MIN_Y + lo[16:24], CROWD_MAX_Y - hi[24:]])
    ox = CROWD_MAX_X - rng.uniform(0, 4.49, 32)               # (max_x - 4.5, max_x]: rounds to column 64
    ox[0] = CROWD_MAX_X
    oy = rng.uniform(20, CROWD_H - 20, 32)
    x = np.concatenate([cx, bx, ox]).astype(np.float32)
    y = np.concatenate([cy, by, oy]).astype(np.float32)
    n = x.shape[0]
    kind = np.concatenate([np.zeros(n_crowd, np.int8), np.ones(32, np.int8), np.full(32, 2, np.int8)])
    perm = rng.permutation(n)
    x, y, kind = x[perm], y[perm], kind[perm]
    octave = rng.integers(2, 4, n).astype(np.int32)
    desc = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    u_right = np.where(rng.random(n) < 0.5, x - rng.uniform(2, 40, n), -1).astype(np.float32)
    F = FrameView(x, y, octave, u_right, desc, CROWD_MIN_X, CROWD_MIN_Y, 64.0 / (CROWD_MAX_X - CROWD_MIN_X),
                  48.0 / (CROWD_MAX_Y - CROWD_MIN_Y), scale)
    return F, dict(crowd=np.nonzero(kind == 0)[0], border=np.nonzero(kind == 1)[0], outside=np.nonzero(kind == 2)[0])


def make_crowd_case(seed, n_crowd=256):
    """Map points over make_crowd_frame: 64 re-observe crowd keypoints, 32 border keypoints (windows clipped at the
    four borders), 8 have windows wholly left of / right of / above / below the grid."""
    from plvs_amd.orbmatcher import MapPointView
    F, sets = make_crowd_frame(seed, n_crowd)
    rng = np.random.default_rng(seed + 1000)
    n = F.x.shape[0]
    src = np.concatenate([rng.choice(sets["crowd"], 64), rng.choice(sets["border"], 32), rng.choice(sets["crowd"], 8)])
    m = src.shape[0]
    px = (F.x[src] + rng.normal(0, 1.5, m)).astype(np.float32)
    py = (F.y[src] + rng.normal(0, 1.5, m)).astype(np.float32)
    px[96:98], px[98:100] = CROWD_MIN_X - 200, CROWD_MAX_X + 200
    py[100:102], py[102:104] = CROWD_MIN_Y - 200, CROWD_MAX_Y + 200
    depth = rng.uniform(0.5, 45.0, m)
    depth[96:] = rng.uniform(0.5, 30.0, 8)                    # (the far-point cut leaves the outside windows in)
    order = rng.permutation(m)
    src, px, py, depth = src[order], px[order], py[order], depth[order]
    M = MapPointView(track_in_view=np.ones(m, np.uint8), bad=np.zeros(m, np.uint8), proj_x=px, proj_y=py,
                     proj_xr=np.where(F.u_right[src] > 0, F.u_right[src] + rng.uniform(-2, 2, m), -1),
                     view_cos=rng.uniform(0.99, 1.0, m), track_depth=depth,
                     level=np.full(m, 3, np.int32), desc=_flip16(rng, F.desc[src]), has_obs=(rng.random(m) < 0.9))
    occupied = (rng.random(n) < 0.05).astype(np.uint8)
    return F, M, occupied, sets


def _c_round(v):
    """std::round of float values (half away from zero), exact in double."""
    v = np.asarray(v, np.float64)
    return np.trunc(v + np.copysign(0.5, v)).astype(np.int64)


def grid_cells(F):
    """Frame::PosInGrid of every keypoint -> (column, row, inside the 64 x 48 grid)."""
    f = np.float32
    px = _c_round((F.x.astype(f) - f(F.min_x)) * f(F.grid_w_inv))
    py = _c_round((F.y.astype(f) - f(F.min_y)) * f(F.grid_h_inv))
    return px, py, (px >= 0) & (px < 64) & (py >= 0) & (py < 48)


def window_counts(F, u, v, r, ur, min_level, max_level):
    """The window test of the searches restated over all keypoints at once: in the grid, |dx| < r, |dy| < r, the level
    band, the stereo gate.  -> (candidates per query [nq], the largest count one query takes from ONE grid column)."""
    f = np.float32
    col, _, inside = grid_cells(F)
    x, y, ku = F.x.astype(f), F.y.astype(f), F.u_right.astype(f)
    u, v, r, ur = (np.asarray(a, f)[:, None] for a in (u, v, r, ur))
    ok = inside[None, :] & (np.abs(x[None, :] - u) < r) & (np.abs(y[None, :] - v) < r)
    ok &= (F.octave[None, :] >= np.asarray(min_level)[:, None]) & (F.octave[None, :] <= np.asarray(max_level)[:, None])
    ok &= ~((ku[None, :] > 0) & (np.abs(ur - ku[None, :]) > r))
    per_col = max((int(ok[:, col == c].sum(1).max()) for c in np.unique(col[inside])), default=0)
    return ok.sum(1), per_col


def crowd_window_counts(F, M, th, far, th_far):
    """window_counts over the map points SearchByProjection processes -> (nq, per query, per column)."""
    f = np.float32
    go = M.track_in_view.astype(bool) & ~M.bad.astype(bool)
    if far:
        go &= ~(M.track_depth.astype(f) > f(th_far))
    r = np.where(M.view_cos.astype(np.float64) > 0.998, f(2.5), f(4.0)).astype(f)
    if th != 1.0:
        r = r * f(th)
    r = (r * F.scale_factors[M.level]).astype(f)
    per_q, per_col = window_counts(F, M.proj_x[go], M.proj_y[go], r[go], M.proj_xr[go], M.level[go] - 1, M.level[go])
    return int(go.sum()), per_q, per_col


def check_crowd_conditions(F, sets, nq, per_q, per_col, spill, empty_windows=8):
    """What makes the case enter the branches it is for."""
    col, row, inside = grid_cells(F)
    assert int((~inside).sum()) == 32 and np.array_equal(np.nonzero(~inside)[0], sets["outside"])
    assert (col[sets["outside"]] == 64).all()
    cells = np.bincount((col * 48 + row)[inside], minlength=64 * 48)
    assert cells.max() > 64                                   # one cell alone is longer than a wave
    assert per_col > 64                                       # second ballot trip WITH accepted members behind the first
    assert (per_q == 0).sum() >= empty_windows                # the windows wholly outside the grid
    if spill:
        assert int(per_q.sum()) > 32 * nq + 4096              # more than the first launch has room for


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_oracle_crowd_case_properties(oracle, seed):
    F, M, occ, sets = make_crowd_case(seed)
    for th, far in ((1.0, False), (5.0, False), (5.0, True)):
        nq, per_q, per_col = crowd_window_counts(F, M, th, far, 40.0)
        check_crowd_conditions(F, sets, nq, per_q, per_col, spill=th >= 3)
        n, a = oracle_search(oracle.lib, F, M, th, far, 40.0, 0.8, occ)
        assert n >= 40 and (a[sets["outside"]] == -1).all()
        assert not occ[a >= 0].any()
        assert (a[sets["border"]] >= 0).sum() >= 8            # clipped windows still find their keypoints
    # th = 1 spills with a larger crowd
    F, M, occ, sets = make_crowd_case(seed, n_crowd=320)
    nq, per_q, per_col = crowd_window_counts(F, M, 1.0, False, 40.0)
    check_crowd_conditions(F, sets, nq, per_q, per_col, spill=True)


@pytest.mark.gpu
@pytest.mark.parametrize("far", [False, True])
@pytest.mark.parametrize("seed,th,n_crowd", [(1, 1.0, 256), (2, 5.0, 256), (3, 1.0, 320), (1, 5.0, 256)])
def test_hip_search_by_projection_crowd(oracle, seed, th, n_crowd, far):
    """Second ballot trip, spill relaunch (th = 5, or 320 crowd keypoints), clipped and empty windows, keypoints
    outside the grid, min_x / min_y != 0."""
    from plvs_amd.orbmatcher import ORBmatcher
    F, M, occ, sets = make_crowd_case(seed, n_crowd)
    nq, per_q, per_col = crowd_window_counts(F, M, th, far, 40.0)
    check_crowd_conditions(F, sets, nq, per_q, per_col, spill=th >= 3 or n_crowd == 320)
    want_n, want = oracle_search(oracle.lib, F, M, th, far, 40.0, 0.8, occ)
    got_n, got = ORBmatcher(0.8, True).SearchByProjection(F, M, th, far, 40.0, occupied=occ)
    assert got_n == want_n >= 40
    assert np.array_equal(got, want)
    assert (got[sets["outside"]] == -1).all()


@pytest.mark.gpu
def test_hip_hamming_pairs_staged_copy():
    """700 + 700 descriptors are 44 800 bytes and two lists of 20 000 int32 pairs 160 000: the 204 800 bytes of input
    are more than the 96 KB (98 304 bytes) up to which the call reads its inputs in place, so they are copied to the
    device first.  20 000 is no multiple of the 256-thread block, 20 224 = 79 * 256 is; 256 and 257 pairs (46 848 and
    46 880 bytes: read in place) end exactly on and one past a block."""
    from plvs_amd import _lib
    rng = np.random.default_rng(5)
    q = rng.integers(0, 256, (700, 32), dtype=np.uint8)
    t = rng.integers(0, 256, (700, 32), dtype=np.uint8)
    for npairs in (20000, 20224, 256, 257):
        assert (2 * 700 * 32 + 2 * 4 * npairs > 96 * 1024) == (npairs >= 20000)
        pq = rng.integers(0, 700, npairs).astype(np.int32)
        pt = rng.integers(0, 700, npairs).astype(np.int32)
        pq[-1], pt[-1] = 699, 699                             # the last descriptor row of both sets
        d = np.full(npairs + 1, -7, np.int32)
        _lib.check(_lib.lib.plvs_hip_hamming_pairs(_lib.np_ptr(q), 700, _lib.np_ptr(t), 700, _lib.np_ptr(pq),
                                                   _lib.np_ptr(pt), npairs, _lib.np_ptr(d)))
        assert np.array_equal(d[:npairs], np.unpackbits(q[pq] ^ t[pt], axis=1).sum(1))
        assert d[npairs] == -7


# ------------------------------------------------------------------ frame to frame (M2)
def make_ff_case(seed, n=1500, w=640, h=480):
    from plvs_amd.orbmatcher import LastFrameView
    F, _, occ = make_case(seed, n=n, m=1)
    rng = np.random.default_rng(seed + 100)
    cur_angle = rng.uniform(0, 360, n).astype(np.float32)
    nl = 1200
    src = rng.integers(0, n, nl)
    desc = F.desc[src].copy()
    desc ^= (rng.integers(0, 256, (nl, 32), dtype=np.uint8) & rng.integers(0, 256, (nl, 32), dtype=np.uint8)
             & rng.integers(0, 256, (nl, 32), dtype=np.uint8))
    u = (F.x[src] + rng.normal(0, 4.0, nl)).astype(np.float32)
    v = (F.y[src] + rng.normal(0, 4.0, nl)).astype(np.float32)
    far = rng.random(nl) < 0.05
    u[far] += 2000                                   # projections outside the image bounds
    invz = rng.uniform(-0.05, 1.0, nl).astype(np.float32)   # a few behind the camera
    ang = (cur_angle[src] + 20 + rng.normal(0, 6, nl)).astype(np.float32)
    wild = rng.random(nl) < 0.2
    ang[wild] = rng.uniform(0, 360, int(wild.sum()))
    L = LastFrameView(valid=(rng.random(nl) < 0.8), u=u, v=v, invz=invz,
                      octave=np.clip(F.octave[src] + rng.integers(-1, 2, nl), 0, 7), angle=ang, desc=desc,
                      has_obs=(rng.random(nl) < 0.97))
    return F, cur_angle, float(w), float(h), 40.0, L, occ


def oracle_search_ff(lib, F, cur_angle, max_x, max_y, mbf, L, th, fwd, bwd, check, occ):
    fc, lc = F.as_c(), L.as_c()
    assigned = np.full(fc.n, -7, np.int32)
    f = lib.oracle_orb_search_by_projection_ff
    f.restype = ctypes.c_int
    f.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_float, ctypes.c_float, ctypes.c_float, ctypes.c_void_p,
                  ctypes.c_float, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    n = f(ctypes.byref(fc), p(cur_angle), max_x, max_y, mbf, ctypes.byref(lc), th, fwd, bwd, check, p(occ), p(assigned))
    return n, assigned


def test_oracle_search_last_frame_properties(oracle):
    F, ang, mx, my, mbf, L, occ = make_ff_case(2)
    n0, a0 = oracle_search_ff(oracle.lib, F, ang, mx, my, mbf, L, 15.0, 0, 0, 0, occ)
    got = np.nonzero(a0 >= 0)[0]
    assert n0 >= len(got) > 100
    for i2 in got:
        i = a0[i2]
        assert L.valid[i] and L.invz[i] >= 0 and 0 <= L.u[i] <= mx and 0 <= L.v[i] <= my and not occ[i2]
        r = 15.0 * F.scale_factors[L.octave[i]]
        assert abs(F.x[i2] - L.u[i]) < r and abs(F.y[i2] - L.v[i]) < r
        assert L.octave[i] - 1 <= F.octave[i2] <= L.octave[i] + 1
        assert oracle.descriptor_distance(L.desc[i], F.desc[i2]) <= 100
    # the rotation check only removes matches; forward / backward restrict the octave band
    n1, a1 = oracle_search_ff(oracle.lib, F, ang, mx, my, mbf, L, 15.0, 0, 0, 1, occ)
    assert n1 < n0 and set(np.nonzero(a1 >= 0)[0]) <= set(got)
    nf, af = oracle_search_ff(oracle.lib, F, ang, mx, my, mbf, L, 15.0, 1, 0, 0, occ)
    for i2 in np.nonzero(af >= 0)[0]:
        assert F.octave[i2] >= L.octave[af[i2]]
    nb, ab = oracle_search_ff(oracle.lib, F, ang, mx, my, mbf, L, 15.0, 0, 1, 0, occ)
    for i2 in np.nonzero(ab >= 0)[0]:
        assert F.octave[i2] <= L.octave[ab[i2]]


@pytest.mark.gpu
@pytest.mark.parametrize("seed,th,fwd,bwd,check", [(1, 15.0, 0, 0, 1), (2, 7.0, 0, 0, 1), (3, 15.0, 1, 0, 1),
                                                   (4, 30.0, 0, 1, 0)])
def test_hip_search_last_frame_matches_oracle(oracle, seed, th, fwd, bwd, check):
    from plvs_amd.orbmatcher import ORBmatcher
    F, ang, mx, my, mbf, L, occ = make_ff_case(seed)
    want_n, want = oracle_search_ff(oracle.lib, F, ang, mx, my, mbf, L, th, fwd, bwd, check, occ)
    got_n, got = ORBmatcher(0.9, bool(check)).SearchByProjectionLastFrame(F, ang, mx, my, mbf, L, th, bool(fwd),
                                                                         bool(bwd), occupied=occ)
    assert got_n == want_n > 30
    assert np.array_equal(got, want)


# ------------------------------------------------------------------ frame to frame on the crowded frame
def make_crowd_ff_case(seed, n_crowd=256):
    """A last frame over make_crowd_frame: 64 projections into the crowd, 32 onto border keypoints, and hand-placed ones
    exactly ON the bounds (kept: the reference drops u < min or u > max only), one float outside them (dropped), with
    invz exactly 0 (kept: only invz < 0 is dropped)."""
    from plvs_amd.orbmatcher import LastFrameView
    F, sets = make_crowd_frame(seed, n_crowd)
    rng = np.random.default_rng(seed + 2000)
    f = np.float32
    n = F.x.shape[0]
    cur_angle = rng.uniform(0, 360, n).astype(f)
    src = np.concatenate([rng.choice(sets["crowd"], 64), rng.choice(sets["border"], 32), rng.choice(sets["border"], 12)])
    nl = src.shape[0]
    u = (F.x[src] + rng.normal(0, 2.0, nl)).astype(f)
    v = (F.y[src] + rng.normal(0, 2.0, nl)).astype(f)
    invz = rng.uniform(0.02, 1.0, nl).astype(f)
    invz[rng.random(nl) < 0.05] = -0.05                       # behind the camera
    lo_x, hi_x, lo_y, hi_y = f(CROWD_MIN_X), f(CROWD_MAX_X), f(CROWD_MIN_Y), f(CROWD_MAX_Y)
    u[96:104] = [lo_x, lo_x, hi_x, hi_x, np.nextafter(lo_x, f(-np.inf)), np.nextafter(hi_x, f(np.inf)), 100, 500]
    v[96:104] = [100, 300, 100, 300, 200, 200, lo_y, hi_y]
    u[104:108], v[104:108] = [200, 400, 10, 630], [np.nextafter(lo_y, f(-np.inf)), np.nextafter(hi_y, f(np.inf)), 10, 470]
    invz[96:108] = rng.uniform(0.02, 1.0, 12)
    zero = np.concatenate([np.arange(0, 64, 16), [96, 98, 106]])
    invz[zero] = 0.0
    ang = (cur_angle[src] + 20 + rng.normal(0, 6, nl)).astype(f)
    wild = rng.random(nl) < 0.2
    ang[wild] = rng.uniform(0, 360, int(wild.sum()))
    L = LastFrameView(valid=(rng.random(nl) < 0.9), u=u, v=v, invz=invz, octave=rng.integers(2, 4, nl).astype(np.int32),
                      angle=ang, desc=_flip16(rng, F.desc[src]), has_obs=(rng.random(nl) < 0.9))
    L.valid[zero] = True
    L.valid[96:108] = True
    order = rng.permutation(nl)
    for k in ("valid", "u", "v", "invz", "octave", "angle", "desc", "has_obs"):
        setattr(L, k, getattr(L, k)[order])
    occ = (rng.random(n) < 0.05).astype(np.uint8)
    return F, cur_angle, float(CROWD_MAX_X), float(CROWD_MAX_Y), 40.0, L, occ, sets


def crowd_ff_window_counts(F, max_x, max_y, mbf, L, th, fwd, bwd):
    """window_counts over the last-frame keypoints the search processes (src/ORBmatcher.cc:1800-1840)."""
    f = np.float32
    u, v, invz = L.u.astype(f), L.v.astype(f), L.invz.astype(f)
    go = L.valid.astype(bool) & ~(invz < 0) & ~((u < f(F.min_x)) | (u > f(max_x))) & ~((v < f(F.min_y)) | (v > f(max_y)))
    oct_ = L.octave[go]
    lo = oct_ if fwd else (np.zeros_like(oct_) if bwd else oct_ - 1)
    hi = np.full_like(oct_, 2 ** 31 - 1) if fwd else (oct_ if bwd else oct_ + 1)
    r = (f(th) * F.scale_factors[oct_]).astype(f)
    ur = (u[go] - f(mbf) * invz[go]).astype(f)
    per_q, per_col = window_counts(F, u[go], v[go], r, ur, lo, hi)
    return int(go.sum()), per_q, per_col, go


FF_CROWD_FLOOR = 30     # the oracle alone gave 36 .. 71 matches over the twelve settings below (of 88 processed projections)
BOW_SPARSE_FLOOR = 100  # the oracle alone gave 201 .. 277 matches on the valid_frac = 0.3 cases
FF_CROWD = [(seed, th, fwd, bwd, check) for seed, th in ((1, 15.0), (2, 30.0)) for fwd, bwd in ((0, 0), (1, 0), (0, 1))
            for check in (0, 1)]


@pytest.mark.parametrize("seed", [1, 2])
def test_oracle_crowd_ff_case_properties(oracle, seed):
    F, ang, mx, my, mbf, L, occ, sets = make_crowd_ff_case(seed)
    f = np.float32
    on_bound = (L.u == f(F.min_x)) | (L.u == f(mx)) | (L.v == f(F.min_y)) | (L.v == f(my))
    assert on_bound.sum() == 6 and (L.invz == 0).sum() == 7
    for th in (15.0, 30.0):
        for fwd, bwd in ((0, 0), (1, 0), (0, 1)):
            nq, per_q, per_col, go = crowd_ff_window_counts(F, mx, my, mbf, L, th, fwd, bwd)
            assert go[on_bound].all() and go[L.invz == 0].all() and (~go & L.valid.astype(bool)).sum() >= 4
            check_crowd_conditions(F, sets, nq, per_q, per_col, spill=True, empty_windows=0)
            n, a = oracle_search_ff(oracle.lib, F, ang, mx, my, mbf, L, th, fwd, bwd, 0, occ)
            assert n >= FF_CROWD_FLOOR and (a[sets["outside"]] == -1).all() and go[a[a >= 0]].all()
            got = np.nonzero(a >= 0)[0]
            if fwd:
                assert (F.octave[got] >= L.octave[a[got]]).all()
            if bwd:
                assert (F.octave[got] <= L.octave[a[got]]).all()


@pytest.mark.gpu
@pytest.mark.parametrize("seed,th,fwd,bwd,check", FF_CROWD)
def test_hip_search_last_frame_crowd(oracle, seed, th, fwd, bwd, check):
    """The forward / backward level gates on crowded windows, with the spill relaunch, projections on the bounds and
    invz == 0."""
    from plvs_amd.orbmatcher import ORBmatcher
    F, ang, mx, my, mbf, L, occ, sets = make_crowd_ff_case(seed)
    nq, per_q, per_col, _ = crowd_ff_window_counts(F, mx, my, mbf, L, th, fwd, bwd)
    check_crowd_conditions(F, sets, nq, per_q, per_col, spill=True, empty_windows=0)
    want_n, want = oracle_search_ff(oracle.lib, F, ang, mx, my, mbf, L, th, fwd, bwd, check, occ)
    got_n, got = ORBmatcher(0.9, bool(check)).SearchByProjectionLastFrame(F, ang, mx, my, mbf, L, th, bool(fwd),
                                                                         bool(bwd), occupied=occ)
    assert got_n == want_n >= FF_CROWD_FLOOR
    assert np.array_equal(got, want)
    assert (got[sets["outside"]] == -1).all()


# ----------------------------------------------------------------- SearchByBoW (M4)
def make_bow_case(seed, nk=1800, nf=2000, nodes=90, valid_frac=0.8):
    """A key frame and a frame re-observing it: descriptors a few bits apart, the vocabulary node a
    function of the clean descriptor so that most true pairs share a node; some land elsewhere."""
    from plvs_amd.orbmatcher import FeatureVector
    rng = np.random.default_rng(seed)
    base = rng.integers(0, 256, (nk, 32), dtype=np.uint8)
    node_of = (base[:, 0].astype(np.int64) * 7 + base[:, 1]) % nodes * 3 + 10      # sparse, unordered ids
    kf_desc = base.copy()
    src = rng.integers(0, nk, nf)
    f_desc = base[src].copy()
    flips = rng.integers(0, 256, (nf, 32), dtype=np.uint8) & rng.integers(0, 256, (nf, 32), dtype=np.uint8) \
        & rng.integers(0, 256, (nf, 32), dtype=np.uint8)
    f_desc ^= flips                                                               # ~32 bits: around TH_LOW
    exact = rng.random(nf) < 0.3
    f_desc[exact] = base[src[exact]]                                              # exact copies -> ties at 0
    f_node = node_of[src].copy()
    stray = rng.random(nf) < 0.1
    f_node[stray] = rng.integers(0, nodes, int(stray.sum())) * 3 + 10 + rng.integers(0, 2, int(stray.sum()))
    kf_nodes, f_nodes = {}, {}
    for i in rng.permutation(nk):
        kf_nodes.setdefault(int(node_of[i]), []).append(int(i))
    for i in rng.permutation(nf):
        f_nodes.setdefault(int(f_node[i]), []).append(int(i))
    kf_valid = (rng.random(nk) < valid_frac).astype(np.uint8)
    kf_angle = rng.uniform(0, 360, nk).astype(np.float32)
    f_angle = (kf_angle[src] + np.where(rng.random(nf) < 0.8, 25.0, rng.uniform(0, 360, nf))
               + rng.normal(0, 4.0, nf)).astype(np.float32) % np.float32(360.0)
    return FeatureVector(kf_nodes), kf_desc, kf_valid, kf_angle, FeatureVector(f_nodes), f_desc, f_angle


def oracle_search_bow(lib, KV, kd, kv, ka, FV, fd, fa, ratio, check):
    assigned = np.full(fd.shape[0], -7, np.int32)
    f = lib.oracle_orb_search_by_bow
    f.restype = ctypes.c_int
    vp = ctypes.c_void_p
    f.argtypes = [vp, vp, ctypes.c_int, vp, vp, vp, vp, ctypes.c_int, vp, ctypes.c_float, ctypes.c_int, vp]
    kc, fc = KV.as_c(), FV.as_c()
    p = lambda a: a.ctypes.data_as(vp)
    n = f(ctypes.byref(kc), p(kd), kd.shape[0], p(kv), p(ka), ctypes.byref(fc), p(fd), fd.shape[0], p(fa), ratio,
          check, p(assigned))
    return n, assigned


def test_oracle_search_by_bow_properties(oracle):
    KV, kd, kv, ka, FV, fd, fa = make_bow_case(1)
    n0, a0 = oracle_search_bow(oracle.lib, KV, kd, kv, ka, FV, fd, fa, 0.7, 0)
    got = np.nonzero(a0 >= 0)[0]
    assert n0 == len(got) > 300
    node_kf = {int(i): int(KV.node_id[a]) for a in range(len(KV.node_id))
               for i in KV.index[KV.offset[a]:KV.offset[a + 1]]}
    node_f = {int(i): int(FV.node_id[a]) for a in range(len(FV.node_id))
              for i in FV.index[FV.offset[a]:FV.offset[a + 1]]}
    assert len(set(a0[got])) == len(got)                       # a key-frame keypoint is visited once
    for i_f in got:
        k = int(a0[i_f])
        assert kv[k] and node_kf[k] == node_f[int(i_f)]
        assert oracle.descriptor_distance(kd[k], fd[i_f]) <= 50
    # a stricter ratio or the rotation check only removes matches
    n1, a1 = oracle_search_bow(oracle.lib, KV, kd, kv, ka, FV, fd, fa, 0.5, 0)
    assert n1 < n0
    n2, a2 = oracle_search_bow(oracle.lib, KV, kd, kv, ka, FV, fd, fa, 0.7, 1)
    assert 0 < n2 < n0 and set(np.nonzero(a2 >= 0)[0]) <= set(got)
    # no common node -> nothing
    from plvs_amd.orbmatcher import FeatureVector
    n3, a3 = oracle_search_bow(oracle.lib, FeatureVector({1: [0, 1]}), kd, kv, ka, FeatureVector({2: [0, 1]}), fd, fa,
                               0.7, 1)
    assert n3 == 0 and (a3 == -1).all()


@pytest.mark.gpu
@pytest.mark.parametrize("seed,ratio,check", [(1, 0.7, 1), (2, 0.7, 0), (3, 0.9, 1), (4, 0.5, 1)])
def test_hip_search_by_bow_matches_oracle(oracle, seed, ratio, check):
    from plvs_amd import _lib
    from plvs_amd.orbmatcher import FeatureVector, ORBmatcher
    KV, kd, kv, ka, FV, fd, fa = make_bow_case(seed)
    want_n, want = oracle_search_bow(oracle.lib, KV, kd, kv, ka, FV, fd, fa, ratio, check)
    got_n, got = ORBmatcher(ratio, bool(check)).SearchByBoW(KV, kd, kv, ka, FV, fd, fa)
    assert got_n == want_n > 100
    assert np.array_equal(got, want)
    # empty sides, disjoint vocabularies, malformed vectors
    m = ORBmatcher(ratio, bool(check))
    n, a = m.SearchByBoW(KV, kd, kv, ka, FeatureVector({}), fd, fa)
    assert n == 0 and (a == -1).all()
    n, a = m.SearchByBoW(FeatureVector({5: [0]}), kd, kv, ka, FeatureVector({6: [0]}), fd, fa)
    assert n == 0 and (a == -1).all()
    with pytest.raises(_lib.PlvsHipError):
        m.SearchByBoW(FeatureVector({5: [kd.shape[0]]}), kd, kv, ka, FV, fd, fa)      # index out of range


def bow_pair_counts(KV, kv, FV):
    """-> (pairs SearchByBoW forms: over the common nodes, VALID key-frame features x frame features; the bound the
    library reserves room for: all key-frame features x frame features)."""
    kf = {int(i): a for a, i in enumerate(KV.node_id)}
    npairs = bound = 0
    for b, node in enumerate(FV.node_id):
        a = kf.get(int(node))
        if a is None:
            continue
        nf = int(FV.offset[b + 1] - FV.offset[b])
        members = KV.index[KV.offset[a]:KV.offset[a + 1]]
        npairs += int(kv[members].astype(bool).sum()) * nf
        bound += len(members) * nf
    return npairs, bound


def test_oracle_search_by_bow_sparse_case_properties(oracle):
    """valid_frac = 0.3: fewer than half of the announced pairs are formed (the library then sends the two pair lists
    in two copies), while the default case fills more than half (one copy over both)."""
    KV, kd, kv, ka, FV, fd, fa = make_bow_case(1)
    npairs, bound = bow_pair_counts(KV, kv, FV)
    assert npairs * 2 >= bound
    for seed in (1, 2):
        KV, kd, kv, ka, FV, fd, fa = make_bow_case(seed, valid_frac=0.3)
        npairs, bound = bow_pair_counts(KV, kv, FV)
        assert 0 < npairs * 2 < bound
        n, a = oracle_search_bow(oracle.lib, KV, kd, kv, ka, FV, fd, fa, 0.7, 1)
        assert n > BOW_SPARSE_FLOOR and kv[a[a >= 0]].all()


@pytest.mark.gpu
@pytest.mark.parametrize("seed,ratio,check", [(1, 0.7, 1), (2, 0.9, 0)])
def test_hip_search_by_bow_sparse_matches_oracle(oracle, seed, ratio, check):
    from plvs_amd.orbmatcher import ORBmatcher
    KV, kd, kv, ka, FV, fd, fa = make_bow_case(seed, valid_frac=0.3)
    npairs, bound = bow_pair_counts(KV, kv, FV)
    assert 0 < npairs * 2 < bound                             # the two-copy branch of the pair upload
    want_n, want = oracle_search_bow(oracle.lib, KV, kd, kv, ka, FV, fd, fa, ratio, check)
    got_n, got = ORBmatcher(ratio, bool(check)).SearchByBoW(KV, kd, kv, ka, FV, fd, fa)
    assert got_n == want_n > BOW_SPARSE_FLOOR
    assert np.array_equal(got, want)
