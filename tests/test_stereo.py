"""Sparse stereo matching (Frame::ComputeStereoMatches): the oracle's properties on
CPU, and the HIP path against the oracle, bit for bit, through the C ABI."""
import functools

import numpy as np
import pytest

from tests import oracle_lib
from tests.oracle_lib import golden

KITTI_FX, KITTI_BF = 718.856, 386.1448           # Examples_old/Stereo/KITTI00-02.yaml
MB = np.float32(KITTI_BF / KITTI_FX)             # Frame.cc: mb = mbf / fx
NLEVELS, SCALE = 8, 1.2


@pytest.fixture(scope="module")
def oracle():
    return oracle_lib.load()


def scale_tables(nlevels=NLEVELS, factor=SCALE):
    """ORBextractor.cc:455-470: float recurrences."""
    s = [np.float32(1.0)]
    for _ in range(1, nlevels):
        s.append(np.float32(s[-1] * np.float32(factor)))
    s = np.array(s, np.float32)
    return s, (np.float32(1.0) / s).astype(np.float32)


def pair(name):
    if name == "urban1":
        return golden("urban1_1241x376.pgm"), golden("urban1_right_1241x376.pgm")
    if name == "shift17":                            # constant disparity 17 px
        img = golden("aloe_640x480.pgm")
        return np.ascontiguousarray(img[:, :-17]), np.ascontiguousarray(img[:, 17:])
    if name == "swapped":                            # negative disparities: (almost) nothing survives
        return golden("urban1_right_1241x376.pgm"), golden("urban1_1241x376.pgm")
    if name == "same":                               # identical images: every correlation score is 0, so is the median
        img = golden("aloe_640x480.pgm")
        return img, img.copy()
    if name == "hinge":                              # disparity 0 left of column 200, 9 px right of it
        img = golden("aloe_640x480.pgm")
        left = np.ascontiguousarray(img[:, :-9])
        right = left.copy()
        right[:, 200:] = img[:, 9:][:, 200:]
        return left, right
    raise KeyError(name)


def oracle_side(oracle, left, right, nfeatures):
    out = []
    for img in (left, right):
        ex = oracle.orb(nfeatures, SCALE, NLEVELS, 20, 7)
        _, k, d = ex.extract(img)
        out.append((k, d, [ex.level(l) for l in range(NLEVELS)]))
    return out


def test_oracle_recovers_a_known_disparity(oracle):
    left, right = pair("shift17")
    (kl, dl, pl), (kr, dr, pr) = oracle_side(oracle, left, right, 1000)
    s, inv = scale_tables()
    u, z, score, kept = oracle.stereo_matches(kl, dl, kr, dr, pl, pr, s, inv, MB, np.float32(KITTI_BF))
    ok = u >= 0
    assert kept == int(ok.sum()) and kept > 0.5 * kl.shape[0]
    disp = kl["x"][ok] - u[ok]
    assert np.abs(disp - 17.0).max() < 1.5 * s[kl["octave"][ok]].max()
    assert np.median(np.abs(disp - 17.0)) < 0.2
    np.testing.assert_array_equal(z[ok], np.float32(KITTI_BF) / disp.astype(np.float32))
    assert (z[~ok] == -1).all() and (score[ok] >= 0).all()


def test_oracle_on_a_real_pair(oracle):
    left, right = pair("urban1")
    (kl, dl, pl), (kr, dr, pr) = oracle_side(oracle, left, right, 2000)
    s, inv = scale_tables()
    u, z, score, kept = oracle.stereo_matches(kl, dl, kr, dr, pl, pr, s, inv, MB, np.float32(KITTI_BF))
    ok = u >= 0
    assert kept == int(ok.sum()) and kept > 0.25 * kl.shape[0]
    disp = kl["x"][ok] - u[ok]
    assert (disp > 0).all() and (disp < KITTI_FX).all() and (z[ok] > 0).all()
    # the median cut: every survivor's score is below 1.5 * 1.4 * median of the pre-cut scores
    pre = np.sort(score[score >= 0])
    th = np.float32(1.5) * np.float32(1.4) * np.float32(pre[pre.shape[0] // 2])
    assert (score[ok] < th).all() and (score[(score >= 0) & ~ok] >= th).all()
    # nothing on the right -> nothing matched, and no crash on the empty median
    u0, z0, _, kept0 = oracle.stereo_matches(kl, dl, kr[:0], dr[:0], pl, pr, s, inv, MB, np.float32(KITTI_BF))
    assert kept0 == 0 and (u0 == -1).all() and (z0 == -1).all()


@pytest.mark.gpu
@pytest.mark.parametrize("name,nfeatures", [("urban1", 2000), ("shift17", 1000), ("swapped", 1000)])
def test_hip_stereo_matches_oracle(oracle, name, nfeatures):
    from plvs_amd.orb import ORBextractor
    from plvs_amd.stereo import StereoMatcher
    left, right = pair(name)
    (kl, dl, pl), (kr, dr, pr) = oracle_side(oracle, left, right, nfeatures)
    exl, exr = ORBextractor(nfeatures, SCALE, NLEVELS, 20, 7), ORBextractor(nfeatures, SCALE, NLEVELS, 20, 7)
    _, hkl, hdl = exl(left)
    _, hkr, hdr = exr(right)
    assert hkl.tobytes() == kl.tobytes() and hkr.tobytes() == kr.tobytes()       # same front end
    assert hdl.tobytes() == dl.tobytes() and hdr.tobytes() == dr.tobytes()
    s, inv = scale_tables()
    np.testing.assert_array_equal(np.asarray(exl.GetScaleFactors(), np.float32), s)
    sm = StereoMatcher(exl, exr)
    want_u, want_z, _, kept = oracle.stereo_matches(kl, dl, kr, dr, pl, pr, s, inv, MB, np.float32(KITTI_BF))
    got_u, got_z = sm.ComputeStereoMatches(hkl, hdl, hkr, hdr, MB, np.float32(KITTI_BF))
    assert got_u.tobytes() == want_u.tobytes()
    assert got_z.tobytes() == want_z.tobytes()
    if name != "swapped":
        assert kept > 0.25 * kl.shape[0]
    # degenerate inputs
    u0, z0 = sm.ComputeStereoMatches(hkl, hdl, hkr[:0], hdr[:0], MB, np.float32(KITTI_BF))
    assert (u0 == -1).all() and (z0 == -1).all()
    u1, z1 = sm.ComputeStereoMatches(hkl[:0], hdl[:0], hkr, hdr, MB, np.float32(KITTI_BF))
    assert u1.shape == (0,) and z1.shape == (0,)
    # a subset of the left keypoints gives the same per-keypoint candidates, but its own median
    sub = slice(0, kl.shape[0] // 3)
    w_u, w_z, _, _ = oracle.stereo_matches(kl[sub], dl[sub], kr, dr, pl, pr, s, inv, MB, np.float32(KITTI_BF))
    g_u, g_z = sm.ComputeStereoMatches(hkl[sub], hdl[sub], hkr, hdr, MB, np.float32(KITTI_BF))
    assert g_u.tobytes() == w_u.tobytes() and g_z.tobytes() == w_z.tobytes()


@pytest.mark.gpu
def test_hip_stereo_needs_both_pyramids():
    from plvs_amd import _lib
    from plvs_amd.orb import ORBextractor, KP_DTYPE
    from plvs_amd.stereo import StereoMatcher
    sm = StereoMatcher(ORBextractor(500, SCALE, NLEVELS, 20, 7), ORBextractor(500, SCALE, NLEVELS, 20, 7))
    k = np.zeros(4, KP_DTYPE)
    with pytest.raises(_lib.PlvsHipError):
        sm.ComputeStereoMatches(k, np.zeros((4, 32), np.uint8), k, np.zeros((4, 32), np.uint8), 0.5, 380.0)


# ------------------------------------------------------------------ median 0, the zero-disparity clamp, window guards
@functools.lru_cache(maxsize=None)
def oracle_case(name, nfeatures=1000):
    """Extraction of a pair by the oracle, once for all tests that use it (nothing below writes into the arrays)."""
    left, right = pair(name)
    (kl, dl, pl), (kr, dr, pr) = oracle_side(oracle_lib.load(), left, right, nfeatures)
    for a in (kl, dl, kr, dr):
        a.setflags(write=False)
    return left, right, kl, dl, pl, kr, dr, pr


def oracle_run(oracle, case, kl=None, dl=None, kr=None, dr=None):
    _, _, kl0, dl0, pl, kr0, dr0, pr = case
    s, inv = scale_tables()
    pick = lambda a, b: b if a is None else a
    return oracle.stereo_matches(pick(kl, kl0), pick(dl, dl0), pick(kr, kr0), pick(dr, dr0), pl, pr, s, inv, MB,
                                 np.float32(KITTI_BF))


CLAMPED_DEPTH = np.float32(KITTI_BF) / np.float32(0.01)      # mbf / 0.01f of the disparity <= 0 branch


def check_same(u, z, score, kept):
    """Identical images: > 100 keypoints reach the cut with score 0, the median is 0 and `score < 1.5 * 1.4 * 0` cuts all."""
    pre = score[score >= 0]
    assert pre.shape[0] > 100 and np.sort(pre)[pre.shape[0] // 2] == 0
    assert kept == 0 and (u == -1).all() and (z == -1).all()


def check_hinge(kl, u, z, score, kept):
    ok = u >= 0
    assert kept == int(ok.sum()) > 100
    clamped = ok & (z == CLAMPED_DEPTH)
    assert clamped.sum() >= 1                                 # survivors of the disparity <= 0 clamp
    np.testing.assert_array_equal(u[clamped], (kl["x"][clamped].astype(np.float64) - 0.01).astype(np.float32))
    disp = kl["x"][ok & ~clamped] - u[ok & ~clamped]
    assert (disp > 0).all() and (np.abs(disp - 9.0) < 1.5 * 1.2 ** 7).sum() > 100


def border_keypoints(case, seed=0):
    """The extractor's keypoints of the pair with ~40 % of the left and of the right coordinates overwritten by values
    on and next to the borders of the image, and some of those moved to octaves 0, 3 and 7, where the scaled coordinates
    meet the borders of the smaller levels.  Descriptors stay as extracted.  -> (kl, kr, moved-left mask)."""
    left, _, kl0, _, _, kr0, _, _ = case
    h, w = left.shape
    rng = np.random.default_rng(seed)
    kl, kr = kl0.copy(), kr0.copy()
    lx = np.array([0, 3, 5.9, 17, 22.9, w - 1, w - 6, w - 12], np.float32)
    ly = np.array([0, 0.5, 4.9, 6.1, h - 6.5, h - 1, h - 0.01, h, -0.5], np.float32)
    rx = np.array([-0.6, 0, 4, 9.9, 10.6, w - 1, w - 11, w - 12.5], np.float32)   # (-0.6: the strip starts left of column 0)
    ry = np.array([0, 0.5, 4.9, 6.1, h - 6.5, h - 1], np.float32)
    moved = []
    for k, xs, ys in ((kl, lx, ly), (kr, rx, ry)):
        n = k.shape[0]
        m = rng.random(n) < 0.4
        what = rng.integers(0, 3, n)                          # x alone, y alone, both
        mx, my = m & (what != 1), m & (what != 0)
        k["x"][mx] = rng.choice(xs, int(mx.sum()))
        k["y"][my] = rng.choice(ys, int(my.sum()))
        lvl = m & (rng.random(n) < 0.3)
        k["octave"][lvl] = rng.choice([0, 3, 7], int(lvl.sum()))
        moved.append(m)
    assert kl["octave"].min() >= 0 and kl["octave"].max() < NLEVELS and kr["octave"].max() < NLEVELS
    return kl, kr, moved[0]


GUARDS = ("row_neg", "row_past", "no_match", "iniu", "endu", "r0", "r1", "c0", "c1", "strip", "through")


def guard_census(case, kl, kr):
    """How often each early return of the matching of one left keypoint is taken, by a restatement of the tests in
    front of the block correlation (Frame.cc:1821-1905) that follows the best right keypoint of the Hamming search."""
    _, _, _, dl, pl, _, dr, _ = case
    s, inv = scale_tables()
    f = np.float32
    n = dict(row_neg=0, row_past=0, no_match=0, iniu=0, endu=0, r0=0, r1=0, c0=0, c1=0, strip=0, through=0)
    dist = np.unpackbits(dl[:, None, :] ^ dr[None, :, :], axis=2).sum(2)
    rr = (f(2.0) * s[kr["octave"]]).astype(f)
    maxr, minr = np.ceil(kr["y"] + rr), np.floor(kr["y"] - rr)
    maxD = f(np.float32(KITTI_BF) / MB)
    for i in range(kl.shape[0]):
        x, y, o = kl["x"][i], kl["y"][i], int(kl["octave"][i])
        if not y >= 0:
            n["row_neg"] += 1
        if y >= pl[0].shape[0]:
            n["row_past"] += 1
        if not (y > -1 and y < pl[0].shape[0]):
            continue
        row = int(y)
        c = (row >= minr) & (row <= maxr) & (np.abs(kr["octave"] - o) <= 1) & (kr["x"] >= f(x - maxD)) & (kr["x"] <= x)
        if not c.any() or dist[i][c].min() >= 75:
            n["no_match"] += 1
            continue
        best = np.nonzero(c)[0][np.argmin(dist[i][c])]
        rnd = lambda v: f(np.trunc(np.float64(v) + np.copysign(0.5, np.float64(v))))
        su, sv, sr = rnd(f(x * inv[o])), rnd(f(y * inv[o])), rnd(f(kr["x"][best] * inv[o]))
        lh, lw = pl[o].shape
        hit = [k for k, bad in (("iniu", sr < 0), ("endu", sr + 11 >= lw), ("r0", sv - 5 < 0), ("r1", sv + 6 > lh),
                                ("c0", su - 5 < 0), ("c1", su + 6 > lw), ("strip", sr - 10 < 0)) if bad]
        for k in hit:
            n[k] += 1
        n["through"] += not hit
    return n


def test_oracle_same_pair_has_median_zero(oracle):
    check_same(*oracle_run(oracle, oracle_case("same")))


def test_oracle_hinge_pair_clamps_zero_disparity(oracle):
    case = oracle_case("hinge")
    check_hinge(case[2], *oracle_run(oracle, case))


def test_oracle_border_keypoints_take_every_guard(oracle):
    case = oracle_case("shift17")
    kl, kr, moved = border_keypoints(case)
    n = guard_census(case, kl, kr)
    for k in GUARDS:
        assert n[k] > 0, (k, n)
    u, z, score, kept = oracle_run(oracle, case, kl=kl, kr=kr)
    assert kept > 100 and moved.sum() > 300
    h, w = case[0].shape
    ok = u >= 0
    assert ((kl["y"][ok] >= 5) & (kl["y"][ok] < h - 5) & (kl["x"][ok] >= 5) & (kl["x"][ok] < w - 5)).all()


SLICES = [(401, 1), (402, 63), (403, 64), (997, 65)]          # n_left: no multiple of the 4 waves of a block


def sliced(case, n_left, n_right):
    """The first n_left left keypoints against every 15th right keypoint (all levels, not the exact copies of level 0
    alone, whose scores of 0 would give median 0 again)."""
    return case[2][:n_left], case[3][:n_left], case[5][3::15][:n_right], case[6][3::15][:n_right]


@pytest.mark.parametrize("n_left,n_right", SLICES)
def test_oracle_slices_keep_matches(oracle, n_left, n_right):
    case = oracle_case("shift17")
    kl, dl, kr, dr = sliced(case, n_left, n_right)
    assert n_left % 4 != 0 and kl.shape[0] == n_left and kr.shape[0] == n_right
    u, z, score, kept = oracle_run(oracle, case, kl, dl, kr, dr)
    assert (score >= 0).sum() >= 1 and kept == int((u >= 0).sum())
    if n_right > 1:
        assert kept >= 10                                     # the oracle gave 19, 19 and 52


@pytest.fixture(scope="module")
def hip_pairs():
    """Per pair: the two HIP extractors after they processed it (their pyramids stay on the device) and a matcher."""
    made = {}

    def get(name):
        if name not in made:
            from plvs_amd.orb import ORBextractor
            from plvs_amd.stereo import StereoMatcher
            case = oracle_case(name)
            exl, exr = ORBextractor(1000, SCALE, NLEVELS, 20, 7), ORBextractor(1000, SCALE, NLEVELS, 20, 7)
            _, hkl, hdl = exl(case[0])
            _, hkr, hdr = exr(case[1])
            assert hkl.tobytes() == case[2].tobytes() and hkr.tobytes() == case[5].tobytes()
            assert hdl.tobytes() == case[3].tobytes() and hdr.tobytes() == case[6].tobytes()
            made[name] = (case, StereoMatcher(exl, exr))
        return made[name]
    return get


def _hip_run(sm, case, kl=None, dl=None, kr=None, dr=None):
    pick = lambda a, b: b if a is None else a
    return sm.ComputeStereoMatches(pick(kl, case[2]), pick(dl, case[3]), pick(kr, case[5]), pick(dr, case[6]), MB,
                                   np.float32(KITTI_BF))


@pytest.mark.gpu
def test_hip_stereo_same_pair_median_zero(oracle, hip_pairs):
    case, sm = hip_pairs("same")
    want = oracle_run(oracle, case)
    check_same(*want)
    got_u, got_z = _hip_run(sm, case)
    assert got_u.tobytes() == want[0].tobytes() and got_z.tobytes() == want[1].tobytes()
    assert (got_u == -1).all() and (got_z == -1).all()


@pytest.mark.gpu
def test_hip_stereo_hinge_pair_zero_disparity_clamp(oracle, hip_pairs):
    case, sm = hip_pairs("hinge")
    want = oracle_run(oracle, case)
    check_hinge(case[2], *want)
    got_u, got_z = _hip_run(sm, case)
    assert got_u.tobytes() == want[0].tobytes() and got_z.tobytes() == want[1].tobytes()


@pytest.mark.gpu
def test_hip_stereo_border_keypoints(oracle, hip_pairs):
    """Keypoints on and next to the borders of the image and of the pyramid levels: every guard in front of the 11 x 11
    window answers as the oracle's (the oracle restates the reference's cv::Mat::rowRange exception as "no match")."""
    case, sm = hip_pairs("shift17")
    kl, kr, _ = border_keypoints(case)
    n = guard_census(case, kl, kr)
    assert min(n[k] for k in GUARDS) > 0
    want_u, want_z, _, kept = oracle_run(oracle, case, kl=kl, kr=kr)
    assert kept > 100
    got_u, got_z = _hip_run(sm, case, kl=kl, kr=kr)
    assert got_u.tobytes() == want_u.tobytes() and got_z.tobytes() == want_z.tobytes()


@pytest.mark.gpu
@pytest.mark.parametrize("n_left,n_right", SLICES)
def test_hip_stereo_slices(oracle, hip_pairs, n_left, n_right):
    """One wave per left keypoint, the lanes stride over the right ones: a last block that is not full, and right
    sets of one keypoint, one short of a wave, a wave, one more."""
    case, sm = hip_pairs("shift17")
    kl, dl, kr, dr = sliced(case, n_left, n_right)
    want_u, want_z, _, _ = oracle_run(oracle, case, kl, dl, kr, dr)
    got_u, got_z = _hip_run(sm, case, kl, dl, kr, dr)
    assert got_u.shape == (n_left,) and got_u.tobytes() == want_u.tobytes() and got_z.tobytes() == want_z.tobytes()
