"""The stereo part of the frame: Frame::ComputeStereoLineMatches (reference src/Frame.cc:2008-2248, with
LineMatcher::SearchStereoMatchesByKnn inside it) as one launch, and the stereo constructor (:214-398) as one call.  Pinned by the
reference's OWN run on tests/frame_stereo_scenario.py, recorded in tests/golden/frame_stereo_reference.npz by
scripts/make_frame_stereo_golden.py; at other sizes by the numpy restatement that file pins.  Every comparison is equality of
bits."""
import ctypes
import json
import os
import re

import numpy as np
import pytest

from tests import frame_stereo_restatement as R
from tests import frame_stereo_scenario as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
ENTRIES = ("plvs_hip_frame_compute_stereo_line_matches", "plvs_hip_frame_stereo_dev")
LINE_KEYS = ("u_right_start", "depth_start", "u_right_end", "depth_end")
REACHED = ("ratio_test", "distance", "octave", "replaced", "equal_not_replaced", "rotation_bins_cut", "vertical_span", "overlap",
           "ll0_small", "lr0_small", "lines_equal", "disparity_below", "disparity_above", "short_3d", "view_angle", "median_cut")
CAPACITY = 512


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def same(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


def _facts():
    with open(os.path.join(GOLDEN, "frame_stereo_reference_facts.json")) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def scenario():
    inp = S.inputs()
    g = np.load(os.path.join(GOLDEN, "frame_stereo_reference.npz"))
    assert S.inputs_digest(inp) == str(g["inputs_digest"]), "the synthetic inputs changed: regenerate with scripts/make_frame_stereo_golden.py"
    return inp, {k: g[k] for k in g.files}


def _lines(inp):
    return inp["keylines"], inp["desc"], inp["keylines_right"], inp["desc_right"]


# ---------------------------------------------------------------------------------------------------------------- CPU
def test_inputs_digest_matches(scenario):
    inp, g = scenario
    assert _facts()["inputs"] == S.inputs_digest(inp) == str(g["inputs_digest"])
    assert len(inp["keylines"]) == 96 == len(g["depth_start"]) and 76 <= len(inp["keylines_right"]) <= 88
    assert sorted(set(inp["keylines"]["octave"])) == [0, 1, 2]


def test_restatement_equals_the_reference(scenario):
    inp, g = scenario
    counters = {}
    out = R.stereo_line_matches(*_lines(inp), *S.args_of(inp), counters=counters)
    for k, o in zip(LINE_KEYS, out):
        assert same(o, g[k]), k
    facts = _facts()["facts"]
    assert {k: facts[k] for k in R.BRANCHES} == counters
    assert out[4] == facts["stereo"] == int((g["depth_start"] > 0).sum())


def test_the_golden_run_takes_every_branch(scenario):
    inp, _ = scenario
    facts = _facts()["facts"]
    for k in REACHED:
        assert facts[k] >= 1, (k, facts[k])
    assert facts["stereo"] >= 8
    assert facts["flag_matched_right"] == 0 == facts["octave_pm1"] and set(facts["unreachable"]) == {"flag_matched_right", "octave_pm1"}
    # the query whose two neighbours are equally far: the multi-index-hash order names another right line than the lowest index
    tie = facts["mih_tie"]
    idx, dist, low = R.knn2_mih(inp["desc"][tie["query"]:tie["query"] + 1], inp["desc_right"])
    assert dist[0, 0] == dist[0, 1] == tie["distance"]
    assert idx[0, 0] == tie["first_neighbour_multi_index_hash"] != tie["first_neighbour_lowest_index"] == low[0, 0]


def test_header_declares_and_library_exports_the_entries():
    with open(os.path.join(ROOT, "include", "plvs_hip.h")) as f:
        header = f.read()
    assert "Frame glue, stereo" in header and "plvs_stereo_calib" in header and "plvs_stereo_frame" in header
    from plvs_amd import _lib      # (loads the library the way the package does: after torch, one HIP runtime per process)
    assert os.path.samefile(_lib.LIB_PATH, os.path.join(ROOT, "plvs_amd", "lib", "libplvs_hip.so"))
    lib = _lib.lib
    for name in ENTRIES:
        assert re.search(r"\bint " + name + r"\(", header), f"{name} is not declared in include/plvs_hip.h"
        assert hasattr(lib, name), f"libplvs_hip.so does not export {name}"
    lib.plvs_hip_abi_version.restype = ctypes.c_int
    assert lib.plvs_hip_abi_version() == 1
    from plvs_amd import frame
    assert callable(frame.compute_stereo_line_matches) and callable(frame.frame_stereo)


# ---------------------------------------------------------------------------------------------------------------- GPU
def _check(got, want):
    assert len(got) == len(want)
    for k, (a, b) in enumerate(zip(got, want)):
        if isinstance(b, (int, np.integer)):
            assert a == b, k
        else:
            assert same(np.asarray(a), np.asarray(b)), k


def _restated(kl, desc, klr, desc_r, **kw):
    args = dict(sigma2=S.LEVEL_SIGMA2, K4=S.K4, mbf=S.MBF, line_stereo_max_dist=S.LINE_STEREO_MAX_DIST, min_line_length_3d=0.01)
    args.update(kw)
    return R.stereo_line_matches(kl, desc, klr, desc_r, **args)


def _device(kl, desc, klr, desc_r, **kw):
    from plvs_amd import frame
    args = dict(line_level_sigma2=S.LEVEL_SIGMA2, K=S.K4, mbf=S.MBF, line_stereo_max_dist=S.LINE_STEREO_MAX_DIST, min_line_length_3d=0.01)
    args.update(kw)
    return frame.compute_stereo_line_matches(kl, desc, klr, desc_r, **args)


@pytest.mark.gpu
def test_line_call_equals_the_reference(scenario):
    from plvs_amd import frame
    from plvs_amd.lines import KEYLINE_DTYPE
    assert KEYLINE_DTYPE == S.KEYLINE_DTYPE
    inp, g = scenario
    got = frame.compute_stereo_line_matches(*_lines(inp), *S.args_of(inp))
    _check(got, tuple(g[k] for k in LINE_KEYS) + (_facts()["facts"]["stereo"],))


@pytest.mark.gpu
def test_matcher_stage_agrees_with_search_stereo_by_knn(scenario):
    """The kernel's holders against plvs_hip_lines_search_stereo_by_knn (device k-NN + the host's order-dependent pass)."""
    from plvs_amd import frame
    from plvs_amd.linematcher import LineMatcher
    inp, _ = scenario
    cases = [(_lines(inp), 0.7, True), (_lines(inp), 0.7, False), (_lines(inp), 1.5, True), (S.random_inputs(100, 100, 11), 0.7, True),
             (S.random_inputs(65, 63, 12, flips=(20, 60)), 0.9, True)]
    for (kl, desc, klr, desc_r), ratio, ori in cases:
        n_valid, matches, valid = LineMatcher(ratio, ori).SearchStereoMatchesByKnn(desc, kl["angle"], kl["octave"], desc_r, klr["angle"],
                                                                                    klr["octave"], 50)
        h = _device(kl, desc, klr, desc_r, nn_ratio=ratio, check_orientation=ori, holders=True)[5]
        held = np.flatnonzero(h[:, 0] >= 0)
        order = held[np.argsort(h[held, 3], kind="stable")]          # vMatches: by the lowest passing query that named the line
        assert list(order) == list(matches["trainIdx"])
        assert list(h[order, 0]) == list(matches["queryIdx"]) and list(h[order, 1]) == [int(d) for d in matches["distance"]]
        assert list(h[order, 2].astype(bool)) == list(valid) and int(h[:, 2].sum()) == n_valid
        assert len(matches) > 10
    # nn_ratio > 1 lets the query with two equally far neighbours through: it holds the line the multi-index hash finds first
    tie = _facts()["facts"]["mih_tie"]
    h = _device(*_lines(inp), nn_ratio=1.5, holders=True)[5]
    assert h[tie["first_neighbour_multi_index_hash"], 0] == tie["query"] and h[tie["first_neighbour_lowest_index"], 0] == -1


@pytest.mark.gpu
def test_result_does_not_depend_on_the_order_of_the_queries(scenario):
    inp, g = scenario
    kl, desc, klr, desc_r = _lines(inp)
    perm = np.random.default_rng(3).permutation(len(kl))
    args = dict(min_line_length_3d=inp["min_line_length_3d"])
    got = _device(kl[perm], desc[perm], klr, desc_r, **args)
    _check(got, _restated(kl[perm], desc[perm], klr, desc_r, **args))
    # where no right line is named twice at one distance by lines that swapped places, the outputs are the permuted golden ones
    # apart from the equal-distance holders (lowest index holds): compare the set of lines with depth outside those groups
    equal = {q for a, b, _ in inp["where"]["equal"] for q in (a, b)}
    keep = np.array([q not in equal for q in perm])
    for k, o in zip(LINE_KEYS, got):
        assert same(o[keep], g[k][perm][keep]), k
    rperm = np.random.default_rng(4).permutation(len(klr))
    _check(_device(kl, desc, klr[rperm], desc_r[rperm], **args)[:4], tuple(g[k] for k in LINE_KEYS))


@pytest.mark.gpu
@pytest.mark.parametrize("n,n_right", [(1, 1), (2, 1), (1, 2), (63, 65), (65, 63), (64, 64), (100, 100), (CAPACITY, CAPACITY)])
def test_sizes_against_the_restatement(n, n_right):
    kl, desc, klr, desc_r = S.random_inputs(n, n_right, seed=100 + n + 7 * n_right)
    counters = {}
    want = _restated(kl, desc, klr, desc_r, counters=counters)
    _check(_device(kl, desc, klr, desc_r), want)
    if min(n, n_right) >= 63:
        assert 10 <= want[4] < min(n, n_right) - 10      # (the distance test, the window and the median cut all bite)
        assert counters["distance"] and counters["disparity_below"] and counters["median_cut"]


@pytest.mark.gpu
def test_empty_sides_and_capacity():
    from plvs_amd import _lib, frame
    kl, desc, klr, desc_r = S.random_inputs(5, 4, seed=1)
    minus = np.full(5, -1, np.float32)
    _check(_device(kl, desc, klr[:0], desc_r[:0]), (minus,) * 4 + (0,))
    _check(_device(kl[:0], desc[:0], klr, desc_r), (minus[:0],) * 4 + (0,))
    _check(_device(kl[:0], desc[:0], klr[:0], desc_r[:0]), (minus[:0],) * 4 + (0,))
    # capacity + 1 on either side: PLVS_ERR_CAPACITY, the outputs untouched
    L = _lib.lib
    p = _lib.np_ptr
    big = S.random_inputs(CAPACITY + 1, CAPACITY + 1, seed=2)
    s2, K4 = S.LEVEL_SIGMA2.copy(), S.K4.copy()
    for n, nr in ((CAPACITY + 1, 3), (3, CAPACITY + 1), (CAPACITY + 1, CAPACITY + 1)):
        out = [np.full(n, 77.0, np.float32) for _ in range(4)]
        ns = ctypes.c_int(-5)
        rc = L.plvs_hip_frame_compute_stereo_line_matches(p(big[0]), p(big[1]), n, p(big[2]), p(big[3]), nr, p(s2), 3, p(K4), float(S.MBF), 20.0,
                                                          0.01, 0.7, 1, 50, *[p(o) for o in out], ctypes.byref(ns), None)
        assert rc == _lib.PLVS_ERR_CAPACITY and ns.value == -5 and all((o == 77.0).all() for o in out)
    assert frame.STEREO_LINE_CAPACITY == CAPACITY


def _single_pair(flips, seed):
    """One left and one right line that triangulate, `flips` bits apart, plus noise lines that match nothing."""
    kl, desc, klr, desc_r = S.random_inputs(6, 6, seed=seed)
    rng = np.random.default_rng(seed)
    desc, desc_r = rng.integers(0, 256, desc.shape, dtype=np.uint8), rng.integers(0, 256, desc_r.shape, dtype=np.uint8)
    q = 0      # its partner: the right line on the same rows
    t = int(np.flatnonzero((klr["startPointY"] == kl["startPointY"][q]) & (klr["endPointY"] == kl["endPointY"][q]))[0])
    desc_r[t] = desc[q]
    for b in rng.permutation(256)[:flips]:
        desc_r[t, b // 8] ^= np.uint8(1 << (b % 8))
    klr["octave"][t], klr["angle"][t] = kl["octave"][q], kl["angle"][q]
    return kl, desc, klr, desc_r, q


@pytest.mark.gpu
def test_median_cut_with_no_and_with_one_survivor():
    # all matches rejected before the median: every pair's right line sits 0.5 px beside the left one (areLinesEqual)
    kl, desc, klr, desc_r = S.random_inputs(40, 40, seed=21)
    same_rows = {(float(a), float(b)): i for i, (a, b) in enumerate(zip(klr["startPointY"], klr["endPointY"]))}
    for q in range(len(kl)):
        t = same_rows[(float(kl["startPointY"][q]), float(kl["endPointY"][q]))]
        klr["startPointX"][t], klr["endPointX"][t] = kl["startPointX"][q] - np.float32(0.5), kl["endPointX"][q] - np.float32(0.5)
    counters = {}
    want = _restated(kl, desc, klr, desc_r, counters=counters)
    assert want[4] == 0 and counters["lines_equal"] >= 30 and counters["median_cut"] == 0
    _check(_device(kl, desc, klr, desc_r), want)
    # exactly one survivor: the median is its own distance d, and the cut removes it iff d >= 2.22f * d — only at d = 0
    for flips, survives in ((0, False), (1, True), (7, True), (49, True)):
        kl, desc, klr, desc_r, q = _single_pair(flips, seed=30 + flips)
        counters = {}
        want = _restated(kl, desc, klr, desc_r, counters=counters)
        assert counters["median_cut"] == (0 if survives else 1) and want[4] == (1 if survives else 0), (flips, counters)
        assert (want[1][q] > 0) == survives
        _check(_device(kl, desc, klr, desc_r), want)


@pytest.mark.gpu
def test_bad_arguments_are_refused():
    import torch
    from plvs_amd import _lib, frame
    from plvs_amd.lines import LineExtractor
    from plvs_amd.orb import ORBextractor
    from plvs_amd.stereo import StereoMatcher
    L = _lib.lib
    p = _lib.np_ptr
    kl, desc, klr, desc_r = S.random_inputs(8, 7, seed=5)
    s2, K4 = S.LEVEL_SIGMA2.copy(), S.K4.copy()
    o = [np.full(8, 77.0, np.float32) for _ in range(4)]

    def call(**kw):
        return L.plvs_hip_frame_compute_stereo_line_matches(
            kw.get("kl", p(kl)), kw.get("desc", p(desc)), kw.get("n", 8), kw.get("klr", p(klr)), kw.get("desc_r", p(desc_r)), kw.get("nr", 7),
            kw.get("s2", p(s2)), kw.get("levels", 3), kw.get("K4", p(K4)), float(S.MBF), 20.0, 0.01, 0.7, 1, 50, kw.get("out", p(o[0])), p(o[1]),
            p(o[2]), kw.get("out_last", p(o[3])), None, None)

    assert call() == _lib.PLVS_OK
    for a in o:
        a[:] = 77.0
    high, neg = kl.copy(), klr.copy()
    high["octave"][5] = 3
    neg["octave"][2] = -1
    bad = [call(n=-1), call(nr=-1), call(kl=None), call(desc=None), call(klr=None), call(desc_r=None), call(s2=None), call(K4=None),
           call(out=None), call(out_last=None), call(levels=0), call(kl=p(high)), call(klr=p(neg)), call(levels=2)]
    assert bad == [_lib.PLVS_ERR_INVALID_ARG] * len(bad)
    assert all((a == 77.0).all() for a in o), "a refused call wrote an output"
    # the one-call entry: a non-rectified calibration, a plvs_stereo made from other handles, one line extractor only
    orb_l, orb_r, orb_x = (ORBextractor(500, 1.2, 8, 20, 7) for _ in range(3))
    lines_l = LineExtractor(50)
    good, other = StereoMatcher(orb_l, orb_r), StereoMatcher(orb_l, orb_x)
    img = torch.zeros((48, 64), dtype=torch.uint8, device="cuda")
    kw = dict(K=S.K4, mbf=S.MBF, bounds=(0, 64, 0, 48), grid_w_inv=1.0, grid_h_inv=1.0)
    for args, dist in (((orb_l, orb_r, None, None, good), (0.1, 0, 0, 0)),        # not rectified
                       ((orb_l, orb_r, None, None, other), None),                 # a plvs_stereo of other handles
                       ((orb_r, orb_l, None, None, good), None),                  # ... of these, swapped
                       ((orb_l, orb_r, None, None, None), None)):
        with pytest.raises(_lib.PlvsHipError) as e:
            frame.frame_stereo(*args, img, img, dist=dist, **kw)
        assert e.value.code == _lib.PLVS_ERR_INVALID_ARG
    # one line extractor only (the mirror cannot say that: straight through the ABI), and no output arrays
    c, f = frame.StereoCalib(), frame.StereoFrameC()
    ip = ctypes.c_void_p(img.data_ptr())
    bad = [L.plvs_hip_frame_stereo_dev(orb_l._h, orb_r._h, lines_l._h, None, good._h, ip, ip, 64, 48, 64, ctypes.byref(c), ctypes.byref(f), None),
           L.plvs_hip_frame_stereo_dev(orb_l._h, orb_r._h, None, None, good._h, ip, ip, 64, 48, 64, ctypes.byref(c), ctypes.byref(f), None),
           L.plvs_hip_frame_stereo_dev(orb_l._h, orb_r._h, None, None, good._h, ip, ip, 64, 48, 63, ctypes.byref(c), ctypes.byref(f), None),
           L.plvs_hip_frame_stereo_dev(orb_l._h, orb_r._h, None, None, good._h, ip, None, 64, 48, 64, ctypes.byref(c), ctypes.byref(f), None)]
    assert bad == [_lib.PLVS_ERR_INVALID_ARG] * len(bad)


# ---- the constructor in one call against the separate entries in the constructor's order
KITTI_K = (718.856, 718.856, 607.1928, 185.2157)      # Examples_old/Stereo/KITTI00-02.yaml
KITTI_BF = 386.1448


def _line_level_sigma2(n_levels, scale):
    s = [np.float32(1.0)]
    for _ in range(1, n_levels):
        s.append(np.float32(s[-1] * np.float32(scale)))
    s = np.array(s, np.float32)
    return (s * s).astype(np.float32)


def _separate(orb_l, orb_r, lines_l, lines_r, stereo, left, right, bounds4, gw, gh, sigma2):
    """The entries one by one, in the order of src/Frame.cc:314-397."""
    from plvs_amd import frame
    if lines_l is not None:
        mono, kps, desc, kl, kld = frame.extract_frame(orb_l, lines_l, left)
        _, kr, dr, klr, kldr = frame.extract_frame(orb_r, lines_r, right)
    else:
        mono, kps, desc = orb_l(left)
        _, kr, dr = orb_r(right)
        kl = klr = np.zeros(0, S.KEYLINE_DTYPE)
        kld = kldr = np.zeros((0, 32), np.uint8)
    out = dict(mono_index=mono, keys=kps, descriptors=desc, keys_right=kr, descriptors_right=dr, keylines=kl, line_descriptors=kld,
               keylines_right=klr, line_descriptors_right=kldr)
    if len(kps) == 0:
        return None
    out["keys_un"] = frame.UndistortKeyPoints(kps, KITTI_K, None)
    mbf = np.float32(KITTI_BF)
    out["u_right"], out["depth"] = stereo.ComputeStereoMatches(kps, desc, kr, dr, mbf / np.float32(KITTI_K[0]), mbf)
    out["n_stereo_points"] = int((out["depth"] > 0).sum())
    if len(kl):
        # UndistortKeyLines on a rectified pair: its early return, mvKeyLinesUn = mvKeyLines (no filter, no compaction)
        out["keylines_un"], out["keylines_right_un"] = kl.copy(), klr.copy()
        *ls, ns = frame.compute_stereo_line_matches(kl, kld, klr, kldr, sigma2, KITTI_K, mbf)
    else:
        out["keylines_un"], out["keylines_right_un"] = kl.copy(), klr[:0].copy()
        ls, ns = [np.zeros(0, np.float32) for _ in range(4)], 0
    out.update(dict(zip(LINE_KEYS, ls)), n_stereo_lines=ns)
    out["cell_start"], out["cell_items"] = frame.AssignFeaturesToGrid(out["keys_un"], bounds4[0], bounds4[2], gw, gh)
    return out


def _same_frame(a, b):
    assert sorted(a) == sorted(b)
    for k in a:
        x, y = np.asarray(a[k]), np.asarray(b[k])
        assert x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes(), k


@pytest.mark.gpu
def test_one_call_constructor_equals_the_separate_entries():
    import torch
    from plvs_amd import frame
    from plvs_amd.lines import LineExtractor
    from plvs_amd.orb import ORBextractor
    from plvs_amd.stereo import StereoMatcher
    from tests.oracle_lib import golden
    gl, gr = golden("urban1_1241x376.pgm"), golden("urban1_right_1241x376.pgm")
    h, w = gl.shape
    assert (h, w) == (376, 1241) == gr.shape
    left, right = torch.from_numpy(gl).cuda(), torch.from_numpy(gr).cuda()
    b = frame.ComputeImageBounds(w, h, KITTI_K, None)
    gw, gh = np.float32(64) / (np.float32(b[1]) - np.float32(b[0])), np.float32(48) / (np.float32(b[3]) - np.float32(b[2]))
    orb_l, orb_r = ORBextractor(2000, 1.2, 8, 20, 7), ORBextractor(2000, 1.2, 8, 20, 7)      # KITTI00-02.yaml
    lines_l, lines_r = LineExtractor(100), LineExtractor(100)
    sigma2 = _line_level_sigma2(lines_l.opts.numOctaves, lines_l.opts.scale)
    stereo = StereoMatcher(orb_l, orb_r)
    kw = dict(K=KITTI_K, dist=None, mbf=KITTI_BF, bounds=b[:4], grid_w_inv=gw, grid_h_inv=gh, line_level_sigma2=sigma2)
    for with_lines in (True, False):
        ll, lr = (lines_l, lines_r) if with_lines else (None, None)
        want = _separate(orb_l, orb_r, ll, lr, stereo, left, right, b[:4], gw, gh, sigma2)
        got = frame.frame_stereo(orb_l, orb_r, ll, lr, stereo, left, right, **kw)
        _same_frame(got, want)
        assert len(got["keys"]) > 1000 and len(got["keys_right"]) > 1000 and got["n_stereo_points"] > 300
        assert got["cell_start"][-1] == len(got["cell_items"]) > 1000
        if with_lines:
            assert len(got["keylines"]) > 20 and len(got["keylines_right"]) > 20
            assert got["keylines_un"].tobytes() == got["keylines"].tobytes()      # no filter, no compaction
            print("lines with depth on the urban1 pair:", got["n_stereo_lines"], "of", len(got["keylines"]))
            assert got["n_stereo_lines"] == int((got["depth_start"] > 0).sum()) >= 3
        else:
            for k in ("keylines", "keylines_un", "line_descriptors", "keylines_right", "keylines_right_un", "line_descriptors_right") + LINE_KEYS:
                assert len(got[k]) == 0, k
    # no key points: zero counts, PLVS_OK, before the lines are touched
    blank = torch.zeros((h, w), dtype=torch.uint8, device="cuda")
    got = frame.frame_stereo(orb_l, orb_r, lines_l, lines_r, stereo, blank, blank, **dict(kw, dist=(0.0, 0.0, 0.0, 0.0)))      # (dist[0] == 0: rectified)
    for k in ("keys", "keys_un", "descriptors", "u_right", "depth", "keylines", "keylines_un", "line_descriptors", "cell_items") + LINE_KEYS:
        assert len(got[k]) == 0, k
    assert not got["cell_start"].any() and got["n_stereo_points"] == got["n_stereo_lines"] == 0
