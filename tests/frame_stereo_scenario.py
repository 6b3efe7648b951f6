"""Seeded scenario behind tests/golden/frame_stereo_reference.npz: a rectified KITTI-shaped pair (1241 x 376) with 96 left
and 82 right lines over three octaves for Frame::ComputeStereoLineMatches.  A right descriptor is its left partner's with a
chosen number of bits flipped, so the scene decides who matches whom and at what distance; the geometry of each pair decides
where the triangulation sends it.  Built so that the reference's run takes every reachable branch — ratio test, distance,
octave, a right line named twice (later closer / equal distance / later farther), rotation bins cut and kept, vertical span,
overlap, |ll(0)|, |lr(0)|, equal lines, disparity below / above the window, short 3-D line, view angle, median cut — and one
query whose two neighbours are equally far, in an order only the multi-index hash explains.
scripts/make_frame_stereo_golden.py asserts each on the reference's run (tests/golden/frame_stereo_reference_facts.json)."""
import hashlib

import numpy as np

from tests.frame_rgbd_scenario import KEYLINE_DTYPE

SEED = 20240822
W, H = 1241, 376
K4 = np.array([718.856, 718.856, 607.1928, 185.2157], np.float32)     # fx, fy, cx, cy
MBF = np.float32(386.1448)
LINE_STEREO_MAX_DIST = np.float32(20.0)       # Tracking::skLineStereoMaxDist
MIN_LINE_LENGTH_3D = np.float32(0.25)         # an argument: larger than the shipped 0.01 so that a 20 px line at 3 m is short
NN_RATIO, CHECK_ORIENTATION, DESCRIPTOR_DIST = 0.7, 1, 50
N_LEVELS = 3
LEVEL_SIGMA2 = np.array([1.0, 1.2 * 1.2, 1.2 * 1.2 * 1.2 * 1.2], np.float32)     # mvLineLevelSigma2 at scale 1.2
N_LEFT = 96


def _flip(d, bits):
    """d with the given bit positions (0..255) flipped."""
    out = d.copy()
    for b in bits:
        out[b // 8] ^= np.uint8(1 << (b % 8))
    return out


def _flip_random(rng, d, k):
    return _flip(d, rng.permutation(256)[:k])


class _Builder:
    def __init__(self, rng):
        self.rng = rng
        self.left, self.right = [], []          # dicts: seg (4 floats), octave, angle, desc

    def add_left(self, seg, octave, angle, desc):
        self.left.append(dict(seg=seg, octave=octave, angle=angle, desc=desc))
        return len(self.left) - 1

    def add_right(self, seg, octave, angle, desc):
        self.right.append(dict(seg=seg, octave=octave, angle=angle, desc=desc))
        return len(self.right) - 1

    def random_desc(self):
        return self.rng.integers(0, 256, 32, dtype=np.uint8)

    def segment(self, x0, y0, dx, dy, ds, de):
        """Left segment and the right one its end points' disparities give (same rows)."""
        return (x0, y0, x0 + dx, y0 + dy), (x0 - ds, y0, x0 + dx - de, y0 + dy)

    def pair(self, left_seg, right_seg, octave, flips, octave_right=None, rot=0.0, desc=None):
        rng = self.rng
        d = self.random_desc() if desc is None else desc
        a = rng.uniform(-1.4, 1.4)
        jitter = rng.uniform(-0.02, 0.02)       # rot a little below or above 0: both sides of the wrap at :503
        q = self.add_left(left_seg, octave, a, d)
        t = self.add_right(right_seg, octave if octave_right is None else octave_right, a - rot + jitter, _flip_random(rng, d, flips))
        return q, t

    def good_geometry(self):
        rng = self.rng
        x0, y0 = rng.uniform(300, 1100), rng.uniform(20, 200)
        dy = rng.uniform(80, 150) * (1 if rng.random() < 0.5 else -1)
        dx = rng.uniform(-40, 40)
        ds = float(MBF) / rng.uniform(4.0, 15.0)
        return self.segment(x0, y0 if dy > 0 else y0 + 150, dx, dy, ds, ds * (1 + rng.uniform(-0.02, 0.02)))


def inputs():
    rng = np.random.default_rng(SEED)
    B = _Builder(rng)
    roles = {}
    # pairs that triangulate: 20 with few bits flipped, 4 far enough for the median cut, 10 turned by pi (a second kept bin)
    for i in range(20):
        B.pair(*B.good_geometry(), octave=i % 3, flips=int(rng.integers(2, 14)))
    roles["median_cut"] = [B.pair(*B.good_geometry(), octave=i % 3, flips=32 + 4 * i)[0] for i in range(4)]
    for i in range(10):
        B.pair(*B.good_geometry(), octave=i % 3, flips=int(rng.integers(2, 14)), rot=np.pi)
    # rotation bins that the three maxima cut: two pairs turned by 1 rad (bin 2), one by 2.1 rad (bin 4)
    roles["rotation_cut"] = [B.pair(*B.good_geometry(), octave=0, flips=5, rot=r)[0] for r in (1.0, 1.05, 2.1)]
    # ratio test: two right lines almost equally close
    for i in range(2):
        q, _ = B.pair(*B.good_geometry(), octave=i, flips=10)
        B.add_right(B.right[-1]["seg"], i, 0.3, _flip_random(rng, B.left[q]["desc"], 12))
    # ... and the query whose two neighbours are equally far (10 bits): the first-added right line differs in one bit of each of
    # the bytes 0..9, the second in five bits of byte 30 and five of byte 31 — the multi-index hash finds the second first
    # (its byte 0 matches exactly), "lowest index" the other, which the permutation below is made to put first
    d = B.random_desc()
    ls, rs = B.good_geometry()
    roles["mih_tie"] = B.add_left(ls, 0, 0.1, d)
    roles["mih_tie_spread"] = B.add_right(rs, 0, 0.1, _flip(d, [8 * k + int(rng.integers(0, 8)) for k in range(10)]))
    roles["mih_tie_packed"] = B.add_right(rs, 0, 0.1, _flip(d, [240, 241, 242, 243, 244, 248, 249, 250, 251, 252]))
    # distance >= 50, octave mismatch
    for i in range(3):
        B.pair(*B.good_geometry(), octave=i, flips=55 + 5 * i)
    for i in range(3):
        B.pair(*B.good_geometry(), octave=i, flips=6, octave_right=(i + 1) % 3)
    # one right line named by two queries: (flips of the query added first, of the second) — which of them comes first is
    # decided after the permutation below, see `named_twice`
    named_twice = []
    for _ in range(5):
        ls, rs = B.good_geometry()
        dr = B.random_desc()
        t = B.add_right(rs, 1, 0.2, dr)
        qa = B.add_left(ls, 1, 0.2, dr)
        qb = B.add_left(ls, 1, 0.2, dr)
        named_twice.append((qa, qb, t))
    # the geometry branches (6 bits flipped each)
    g = lambda *a: B.segment(*[float(v) for v in a])                                                 # noqa: E731
    for i in range(2):
        B.pair(*g(400 + 50 * i, 100, 80, 1.5, 40, 40), octave=i, flips=6)                            # left line nearly horizontal
    B.pair((500.0, 100.0, 505.0, 160.0), (460.0, 100.0, 540.0, 101.0), octave=0, flips=6)            # right line nearly horizontal
    for i in range(3):
        B.pair((600.0, 100.0, 610.0, 160.0), (560.0, 159.0 - i, 570.0, 219.0), octave=i, flips=6)    # rows hardly overlap
    for i in range(2):
        B.pair(*g(60, 150 + 10 * i, 1100, 3.2, 40, 40), octave=i * 2, flips=6)                       # |ll(0)| small
    for i in range(2):
        B.pair((700.0, 200.0, 705.0, 260.0), (30.0, 200.0 + i, 1130.0, 203.2 + i), octave=i, flips=6)   # |lr(0)| small
    for i in range(3):
        B.pair(*g(800 + 20 * i, 50, 8, 90, 0.5, 0.5), octave=i, flips=6)                             # the same line in both images
    for i in range(3):
        B.pair(*g(500 + 30 * i, 60, 10, 100, 6, 6 + i), octave=i, flips=6)                           # disparity below the window
    for i in range(2):
        B.pair(*g(1000 + 40 * i, 60, 10, 100, 800, 800 + 10 * i), octave=i, flips=6)                 # ... above it
    for i in range(3):
        B.pair(*g(500 + 60 * i, 120, 5, 20, float(MBF) / 3.0, float(MBF) / 3.0), octave=i, flips=6)  # short in 3-D
    for i in range(3):
        B.pair(*g(450 + 60 * i, 150, 10, 40, float(MBF) / 4.0, float(MBF) / 14.0), octave=i, flips=6)   # along the viewing ray
    # lines without a partner
    while len(B.left) < N_LEFT:
        ls, _ = B.good_geometry()
        B.add_left(ls, int(rng.integers(0, 3)), rng.uniform(-1.4, 1.4), B.random_desc())
    for _ in range(4):
        _, rs = B.good_geometry()
        B.add_right(rs, int(rng.integers(0, 3)), rng.uniform(-1.4, 1.4), B.random_desc())
    # both sides in random order; then the twice-named right lines get their two queries' distances by who comes first
    nl, nr = len(B.left), len(B.right)
    pos_l, pos_r = rng.permutation(nl), rng.permutation(nr)        # line i goes to slot pos[i]
    if pos_r[roles["mih_tie_spread"]] > pos_r[roles["mih_tie_packed"]]:     # the tie: the spread one must come first ("lowest index")
        roles["mih_tie_spread"], roles["mih_tie_packed"] = roles["mih_tie_packed"], roles["mih_tie_spread"]
        a, b = B.right[roles["mih_tie_spread"]], B.right[roles["mih_tie_packed"]]
        a["desc"], b["desc"] = b["desc"], a["desc"]
    plan = ((20, 8, "later_closer"), (22, 9, "later_closer"), (12, 12, "equal"), (15, 15, "equal"), (7, 19, "later_farther"))
    for (qa, qb, t), (first_flips, second_flips, what) in zip(named_twice, plan):
        first, second = (qa, qb) if pos_l[qa] < pos_l[qb] else (qb, qa)
        B.left[first]["desc"] = _flip_random(rng, B.right[t]["desc"], first_flips)
        B.left[second]["desc"] = _flip_random(rng, B.right[t]["desc"], second_flips)
        roles.setdefault(what, []).append((int(pos_l[first]), int(pos_l[second]), int(pos_r[t])))

    def lines(items, pos):
        kl = np.zeros(len(items), KEYLINE_DTYPE)
        desc = np.zeros((len(items), 32), np.uint8)
        for i, it in enumerate(items):
            k = pos[i]
            seg = np.asarray(it["seg"], np.float32)
            kl["startPointX"][k], kl["startPointY"][k], kl["endPointX"][k], kl["endPointY"][k] = seg
            kl["sPointInOctaveX"][k], kl["sPointInOctaveY"][k], kl["ePointInOctaveX"][k], kl["ePointInOctaveY"][k] = seg
            kl["pt_x"][k], kl["pt_y"][k] = (seg[0] + seg[2]) / 2, (seg[1] + seg[3]) / 2
            kl["lineLength"][k] = np.sqrt((seg[2] - seg[0]) ** 2 + (seg[3] - seg[1]) ** 2)
            kl["octave"][k], kl["angle"][k], kl["class_id"][k] = it["octave"], np.float32(it["angle"]), k
            kl["response"][k], kl["size"][k], kl["numOfPixels"][k] = 1.0, 1.0, 10
            desc[k] = it["desc"]
        return kl, desc

    kl, desc = lines(B.left, pos_l)
    klr, desc_r = lines(B.right, pos_r)
    where = dict(median_cut=[int(pos_l[q]) for q in roles["median_cut"]], rotation_cut=[int(pos_l[q]) for q in roles["rotation_cut"]],
                 mih_tie=dict(query=int(pos_l[roles["mih_tie"]]), spread=int(pos_r[roles["mih_tie_spread"]]),
                              packed=int(pos_r[roles["mih_tie_packed"]])),
                 **{k: roles[k] for k in ("later_closer", "equal", "later_farther")})
    return dict(keylines=kl, desc=desc, keylines_right=klr, desc_right=desc_r, level_sigma2=LEVEL_SIGMA2.copy(), K4=K4.copy(), mbf=MBF,
                line_stereo_max_dist=LINE_STEREO_MAX_DIST, min_line_length_3d=MIN_LINE_LENGTH_3D, nn_ratio=NN_RATIO,
                check_orientation=CHECK_ORIENTATION, descriptor_dist=DESCRIPTOR_DIST, where=where)


def inputs_digest(inp):
    h = hashlib.sha1()
    for k in ("keylines", "desc", "keylines_right", "desc_right", "level_sigma2", "K4"):
        h.update(np.ascontiguousarray(inp[k]).tobytes())
    for k in ("mbf", "line_stereo_max_dist", "min_line_length_3d", "nn_ratio"):
        h.update(np.float32(inp[k]).tobytes())
    h.update(np.array([inp["check_orientation"], inp["descriptor_dist"]], np.int32).tobytes())
    return h.hexdigest()


def args_of(inp):
    """Positional arguments of the restatement / the Python mirror after the four line arrays."""
    return (inp["level_sigma2"], inp["K4"], inp["mbf"], inp["line_stereo_max_dist"], inp["min_line_length_3d"], inp["nn_ratio"],
            inp["check_orientation"], inp["descriptor_dist"])


def random_inputs(n, n_right, seed, flips=None):
    """n left and n_right right lines for the size tests: the first min(n, n_right) are partners, placed in random order, the
    others are noise.  Three partners in four are 2 - 9 bits apart, the others 25 - 59 (so the distance test and the median cut
    both bite; flips=(lo, hi) draws all of them from one range); one in ten lies below the disparity window, the others
    triangulate.  Not pinned by the golden file: held to the restatement."""
    rng = np.random.default_rng(seed)
    B = _Builder(rng)
    for i in range(min(n, n_right)):
        lo, hi = flips if flips is not None else ((2, 10) if rng.random() < 0.75 else (25, 60))
        ls, rs = B.good_geometry()
        if rng.random() < 0.1:
            ls, rs = B.segment(ls[0], ls[1], ls[2] - ls[0], ls[3] - ls[1], 5.0, 6.0)
        B.pair(ls, rs, octave=i % 3, flips=int(rng.integers(lo, hi)))
    while len(B.left) < n:
        B.add_left(B.good_geometry()[0], int(rng.integers(0, 3)), rng.uniform(-1.4, 1.4), B.random_desc())
    while len(B.right) < n_right:
        B.add_right(B.good_geometry()[1], int(rng.integers(0, 3)), rng.uniform(-1.4, 1.4), B.random_desc())
    pl, pr = rng.permutation(n), rng.permutation(n_right)
    kl, desc = np.zeros(n, KEYLINE_DTYPE), np.zeros((n, 32), np.uint8)
    klr, desc_r = np.zeros(n_right, KEYLINE_DTYPE), np.zeros((n_right, 32), np.uint8)
    for items, pos, k_, d_ in ((B.left, pl, kl, desc), (B.right, pr, klr, desc_r)):
        for i, it in enumerate(items):
            k = pos[i]
            k_["startPointX"][k], k_["startPointY"][k], k_["endPointX"][k], k_["endPointY"][k] = np.asarray(it["seg"], np.float32)
            k_["octave"][k], k_["angle"][k], k_["class_id"][k] = it["octave"], np.float32(it["angle"]), k
            d_[k] = it["desc"]
    return kl, desc, klr, desc_r
