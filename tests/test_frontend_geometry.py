"""The HIP ORB and line extractors at the shipped sizes and settings and at the cell / tile edges of their kernels
(tests/frontend_cases.py), against the oracle, stage by stage, through the C ABI and its Python mirrors.

Bar: bit-exact everywhere — pyramid levels, FAST candidates, blurred levels, every key-point field (angle by bits),
descriptor bits; octave maps, segments per octave, KeyLine bytes, LBD bits.  The oracle's own output must pass the case's
floor first (frontend_cases.check_*_floor), so no comparison is of nothing.  The same cases pin the oracle by the compiled
reference on the CPU (tests/test_oracle_pinned_frontend.py)."""
import ctypes

import numpy as np
import pytest

from tests import frontend_cases as C
from tests.oracle_lib import KP_DTYPE

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------ ORB
def _assert_orb_equal(got, want, what):
    mono, kps, desc = got
    assert mono == want.mono and len(kps) == len(want.kps), f"{what}: {mono} / {len(kps)} key points, oracle {want.mono} / {len(want.kps)}"
    for f in ("x", "y", "size", "response", "octave", "class_id"):
        assert np.array_equal(kps[f], want.kps[f]), f"{what}: key-point field {f}"
    assert np.array_equal(kps["angle"].view(np.uint32), want.kps["angle"].view(np.uint32)), f"{what}: angle bits"
    assert np.array_equal(desc, want.desc), f"{what}: descriptor bits"


def _assert_orb_stages_equal(dev, got, want, what):
    """pyramid -> candidates -> key points -> angle -> blur -> descriptor: the first stage that differs names itself"""
    for level, lv in enumerate(want.levels):
        assert np.array_equal(dev.level(level), lv), f"{what}: pyramid level {level}"
    for level, cand in enumerate(want.candidates):
        assert np.array_equal(dev.candidates(level), cand), f"{what}: FAST candidates level {level}"
    mono, kps, desc = got
    assert mono == want.mono and len(kps) == len(want.kps), f"{what}: {mono} / {len(kps)} key points, oracle {want.mono} / {len(want.kps)}"
    for f in ("x", "y", "response", "octave"):
        assert np.array_equal(kps[f], want.kps[f]), f"{what}: key-point field {f}"
    assert np.array_equal(kps["angle"].view(np.uint32), want.kps["angle"].view(np.uint32)), f"{what}: angle bits"
    for level, b in enumerate(want.blurred):
        if b is not None:
            assert np.array_equal(dev.level(level, True), b), f"{what}: blurred level {level}"
    _assert_orb_equal(got, want, what)


@pytest.mark.parametrize("case", C.ORB_CASES, ids=[c.id for c in C.ORB_CASES])
def test_hip_orb_case_matches_oracle_stage_by_stage(oracle, case):
    from plvs_amd.orb import ORBextractor
    want = C.oracle_orb(oracle, case)
    C.check_orb_floor(case, want)
    dev = ORBextractor(*case.settings)
    try:
        assert np.array_equal(dev.features_per_level(), want.features_per_level)
        for got_t, want_t in zip(dev._tables(), C.scale_tables(case.settings)):
            assert got_t.tobytes() == want_t.tobytes(), f"{case.id}: scale tables"
        got = dev(C.image(case.image), None, (0, 0))
        _assert_orb_stages_equal(dev, got, want, case.id)
    finally:
        dev.close()


def test_hip_orb_one_handle_over_a_sequence_of_geometries(oracle):
    """Every geometry change rebuilds the level table, the cells, the tap tables and the score map: nothing of the larger
    image before (1280x720), of a one-cell image (67x67) or of an image without any cell (66x66) may survive into the next."""
    from plvs_amd.orb import ORBextractor
    dev = ORBextractor(*C.DEFAULT)
    results = []
    try:
        for name in ("aloe_1280x720", "edge_67x67", "aloe_752x480", "edge_66x66", "aloe_752x480"):
            case = C.orb_case(name)
            want = C.oracle_orb(oracle, case)
            C.check_orb_floor(case, want)
            got = dev(C.image(name))
            _assert_orb_stages_equal(dev, got, want, f"{name} (call {len(results)})")
            results.append(got)
    finally:
        dev.close()
    assert results[4][0] == results[2][0] and results[4][1].tobytes() == results[2][1].tobytes()
    assert np.array_equal(results[4][2], results[2][2])
    assert results[3][0] == 0 and len(results[3][1]) == 0


@pytest.mark.parametrize("name", ["aloe_752x480", "edge_101x67"])
def test_hip_orb_row_pitch(oracle, name):
    """The host entry with stride = w + 13 (the image is a column slice of a wider array whose other bytes are 255) and the
    device entry with a non-contiguous view: both equal the contiguous call and the oracle."""
    import torch
    from plvs_amd import _lib
    from plvs_amd.orb import L, ORBextractor
    case = C.orb_case(name)
    want = C.oracle_orb(oracle, case)
    C.check_orb_floor(case, want)
    img = C.image(name)
    h, w = img.shape
    wide = np.full((h, w + 13), 255, np.uint8)
    wide[:, :w] = img
    dev = ORBextractor(*case.settings)
    try:
        contiguous = dev(img)
        _assert_orb_equal(contiguous, want, f"{name}: contiguous")
        # host entry, called directly (the mirror would make the slice contiguous)
        cap = dev._cap
        kps, desc = np.zeros(cap, KP_DTYPE), np.zeros((cap, 32), np.uint8)
        n, mono = ctypes.c_int(), ctypes.c_int()
        _lib.check(L.plvs_hip_orb_extract(dev._h, _lib.np_ptr(wide), w, h, w + 13, 0, 0, _lib.np_ptr(kps), _lib.np_ptr(desc),
                                          cap, ctypes.byref(n), ctypes.byref(mono)))
        _assert_orb_stages_equal(dev, (mono.value, kps[:n.value], desc[:n.value]), want, f"{name}: host stride w + 13")
        # device entry: a column slice of the wider tensor
        view = torch.from_numpy(wide).cuda()[:, :w]
        assert not view.is_contiguous() and view.stride(0) == w + 13
        _assert_orb_stages_equal(dev, dev(view), want, f"{name}: device stride w + 13")
        # and one that starts inside a row
        wide2 = np.full((h + 2, w + 13), 255, np.uint8)
        wide2[1:h + 1, 5:w + 5] = img
        view2 = torch.from_numpy(wide2).cuda()[1:h + 1, 5:w + 5]
        _assert_orb_equal(dev(view2), want, f"{name}: device view with an offset")
    finally:
        dev.close()


def test_hip_orb_lapping_area_at_752x480(oracle):
    """vLappingArea = (250, 500): the key points inside go to the back, in reverse order (ORBextractor.cc:1357-1378)."""
    from plvs_amd.orb import ORBextractor
    case = C.orb_case("aloe_752x480")
    want = C.oracle_orb(oracle, case, lap=(250, 500))
    C.check_orb_floor(case, want)
    inside = (want.kps["x"] >= 250) & (want.kps["x"] <= 500)
    assert 100 < want.mono < len(want.kps) - 100                 # both parts are populated
    assert not inside[:want.mono].any() and inside[want.mono:].all()
    dev = ORBextractor(*case.settings)
    try:
        _assert_orb_equal(dev(C.image(case.image), None, (250, 500)), want, "lapping area")
    finally:
        dev.close()


# ------------------------------------------------------------------ lines
def _dev_lines(case):
    from plvs_amd.lines import LineExtractor, LSDOptions
    kw = C.LINE_SETTINGS[case.setting]
    return LineExtractor(kw["nfeatures"], LSDOptions(numOctaves=kw["nlevels"], scale=kw["scale"], min_length=kw["min_length"],
                                                     lineFitErrThreshold=kw["fit_err"]))


def _assert_lines_stages_equal(dev, got, ora, want, what, maps=("blur", "dx", "dy", "gd")):
    for o in range(ora.nlevels):                                  # the extractor's own octave count
        w, h = ora.octave_size(o)
        assert dev.octave_map(o, "blur").shape == (h, w), f"{what}: size of octave {o}"
        for which in maps:
            if which == "gd":
                gd = dev.octave_map(o, "gd")
                assert np.array_equal((gd & 0x1ff).astype(np.int16), ora.octave_map(o, "g")), f"{what}: gradient octave {o}"
                assert np.array_equal(np.where(gd & 0x8000, 255, 0), ora.octave_map(o, "dir")), f"{what}: direction octave {o}"
            else:
                assert np.array_equal(dev.octave_map(o, which), ora.octave_map(o, which)), f"{what}: {which} octave {o}"
        assert dev.num_in_octave(o) == ora.num_in_octave(o), f"{what}: segments in octave {o}"
    kl, desc = got
    okl, odesc = want
    assert len(kl) == len(okl), f"{what}: {len(kl)} lines, oracle {len(okl)}"
    assert kl.tobytes() == okl.tobytes(), f"{what}: KeyLine records differ"
    assert np.array_equal(desc, odesc), f"{what}: LBD descriptor bits differ"


def _oracle_lines(oracle, case):
    ora = oracle.lines(**C.LINE_SETTINGS[case.setting])
    want = ora.extract(C.image(case.image))
    C.check_lines_floor(case, want[0])
    return ora, want


DEVICE_INPUT = "aloe_752x480-four"          # this case hands the image over as a device tensor


@pytest.mark.parametrize("case", C.LINE_CASES, ids=[c.id for c in C.LINE_CASES])
def test_hip_lines_case_matches_oracle_stage_by_stage(oracle, case):
    import torch
    ora, want = _oracle_lines(oracle, case)
    dev = _dev_lines(case)
    try:
        img = C.image(case.image)
        got = dev(torch.from_numpy(img.copy()).cuda() if case.id == DEVICE_INPUT else img)
        _assert_lines_stages_equal(dev, got, ora, want, case.id)
    finally:
        dev.close()


def test_hip_lines_one_handle_over_two_sizes_and_a_pitched_device_view(oracle):
    """The 4-octave, 1.5 setting on one handle: 333x181, then 64x48 (every octave shrinks), then 333x181 again — from a
    device view with stride w + 13 — equals the first call."""
    import torch
    big, small = C.line_case("aloe_333x181", "four"), C.line_case("aloe_64x48", "four")
    dev = _dev_lines(big)
    try:
        first = None
        for k, case in enumerate((big, small, big)):
            ora, want = _oracle_lines(oracle, case)
            img = C.image(case.image)
            if k == 2:
                h, w = img.shape
                wide = np.full((h, w + 13), 255, np.uint8)
                wide[:, :w] = img
                img = torch.from_numpy(wide).cuda()[:, :w]
                assert img.stride(0) == w + 13
            got = dev(img)
            _assert_lines_stages_equal(dev, got, ora, want, f"{case.id} (call {k})")
            first = first or got
        assert got[0].tobytes() == first[0].tobytes() and np.array_equal(got[1], first[1])
    finally:
        dev.close()


def test_hip_lines_host_row_pitch(oracle):
    """plvs_hip_lines_extract with stride = w + 13, called directly."""
    from plvs_amd import _lib
    from plvs_amd.lines import KEYLINE_DTYPE, L
    case = C.line_case("aloe_101x67")
    ora, want = _oracle_lines(oracle, case)
    img = C.image(case.image)
    h, w = img.shape
    wide = np.full((h, w + 13), 255, np.uint8)
    wide[:, :w] = img
    dev = _dev_lines(case)
    try:
        kl, desc = np.zeros(4096, KEYLINE_DTYPE), np.zeros((4096, 32), np.uint8)
        n = ctypes.c_int()
        _lib.check(L.plvs_hip_lines_extract(dev._h, _lib.np_ptr(wide), w, h, w + 13, _lib.np_ptr(kl), _lib.np_ptr(desc), 4096,
                                            ctypes.byref(n)))
        _assert_lines_stages_equal(dev, (kl[:n.value], desc[:n.value]), ora, want, "host stride w + 13")
    finally:
        dev.close()


# ------------------------------------------------------------------ shared pyramid, combined entry
def test_hip_shared_pyramid_and_combined_entry_at_752x480(oracle):
    """Line.pyramidPrecomputation at the EuRoC size: the line octaves are the ORB levels (627x400, 522x333: odd sizes the
    640x480 goldens never give), and the combined frame extraction returns what the two extractors return alone."""
    import torch
    from plvs_amd.frame import extract_frame
    from plvs_amd.lines import LineExtractor
    from plvs_amd.orb import ORBextractor
    case = C.orb_case("aloe_752x480")
    img = C.image(case.image)
    want = C.oracle_orb(oracle, case)
    C.check_orb_floor(case, want)
    ol = oracle.lines()
    ol.set_pyramid(want.levels, 3, 1.2)
    okl, oldesc = ol.extract(img)
    assert len(okl) >= 90                                         # measured: 100
    own = C.line_case(case.image)
    oown, own_want = _oracle_lines(oracle, own)
    assert okl.tobytes() != own_want[0].tobytes()                 # the shared pyramid is another input than the own chain
    orb, lines = ORBextractor(*case.settings), LineExtractor(100)
    dimg = torch.from_numpy(img.copy()).cuda()
    try:
        # the two alone, own pyramids; then the combined entry
        _assert_orb_equal(orb(img), want, "ORB alone")
        _assert_lines_stages_equal(lines, lines(img), oown, own_want, "lines alone")
        for k in range(2):
            mono, kps, desc, kl, ldesc = extract_frame(orb, lines, dimg)
            _assert_orb_equal((mono, kps, desc), want, f"combined entry, points (call {k})")
            _assert_lines_stages_equal(lines, (kl, ldesc), oown, own_want, f"combined entry, lines (call {k})")
        # shared: sequential, then through the combined entry
        lines.SetGaussianPyramid(orb)
        orb(img)
        _assert_lines_stages_equal(lines, lines(img), ol, (okl, oldesc), "shared pyramid")
        for k in range(2):
            mono, kps, desc, kl, ldesc = extract_frame(orb, lines, dimg)
            _assert_orb_equal((mono, kps, desc), want, f"combined entry on the shared pyramid, points (call {k})")
            _assert_lines_stages_equal(lines, (kl, ldesc), ol, (okl, oldesc), f"combined entry on the shared pyramid, lines (call {k})")
    finally:
        lines.close()
        orb.close()


# ------------------------------------------------------------------ stereo over a non-default pyramid
def test_hip_stereo_over_a_four_level_pyramid(oracle):
    """Frame::ComputeStereoMatches with extractors (1000, 1.3, 4, 20, 7): the row bands, the search range and the 11x11
    refinement read the scale tables and the pyramid of THAT extractor.  uRight and depth bit-equal.
    Measured on the oracle: 510 of the 1003 left key points keep a match (51 %)."""
    from plvs_amd.orb import ORBextractor
    from plvs_amd.stereo import StereoMatcher
    from tests.test_stereo import KITTI_BF, MB, pair, scale_tables
    settings = (1000, 1.3, 4, 20, 7)
    left, right = pair("shift17")
    sides = []
    for img in (left, right):
        ex = oracle.orb(*settings)
        _, k, d = ex.extract(img)
        sides.append((k, d, [ex.level(l) for l in range(4)]))
    (kl, dl, pl), (kr, dr, pr) = sides
    s, inv = scale_tables(4, 1.3)
    want_u, want_z, _, kept = oracle.stereo_matches(kl, dl, kr, dr, pl, pr, s, inv, MB, np.float32(KITTI_BF))
    print(f"stereo (1000, 1.3, 4): oracle keeps {kept} of {len(kl)} left key points")
    assert len(kl) >= 900 and kept > 0.25 * len(kl)
    assert kept == int((want_u >= 0).sum())
    exl, exr = ORBextractor(*settings), ORBextractor(*settings)
    sm = None
    try:
        _, hkl, hdl = exl(left)
        _, hkr, hdr = exr(right)
        assert hkl.tobytes() == kl.tobytes() and hkr.tobytes() == kr.tobytes()       # same front end
        assert hdl.tobytes() == dl.tobytes() and hdr.tobytes() == dr.tobytes()
        np.testing.assert_array_equal(np.asarray(exl.GetScaleFactors(), np.float32), s)
        np.testing.assert_array_equal(np.asarray(exl.GetInverseScaleFactors(), np.float32), inv)
        sm = StereoMatcher(exl, exr)
        got_u, got_z = sm.ComputeStereoMatches(hkl, hdl, hkr, hdr, MB, np.float32(KITTI_BF))
        assert got_u.tobytes() == want_u.tobytes(), f"uRight differs at {np.flatnonzero(got_u != want_u)[:8]}"
        assert got_z.tobytes() == want_z.tobytes()
    finally:
        if sm is not None:
            sm.close()
        exl.close()
        exr.close()
