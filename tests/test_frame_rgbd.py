"""The RGB-D part of the frame: Frame::ComputeStereoFromRGBD, Frame::ComputeStereoLinesFromRGBD, ComputeSceneMedianDepth
(reference src/Frame.cc:2251-2279, 2434-2674, 2730-2751) and the RGB-D constructor as one call.  Pinned by the reference's OWN
run on tests/frame_rgbd_scenario.py, recorded in tests/golden/frame_rgbd_reference.npz by scripts/make_frame_rgbd_golden.py.
Every comparison is equality of bits."""
import ctypes
import json
import os
import re

import numpy as np
import pytest

from tests import frame_rgbd_restatement as R
from tests import frame_rgbd_scenario as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
ENTRIES = ("plvs_hip_frame_compute_stereo_from_rgbd", "plvs_hip_frame_compute_stereo_lines_from_rgbd",
           "plvs_hip_frame_stereo_from_rgbd_dev", "plvs_hip_frame_scene_median_depth", "plvs_hip_frame_rgbd_dev")
LINE_KEYS = ("u_right_start", "depth_start", "u_right_end", "depth_end")


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def same(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


@pytest.fixture(scope="module")
def scenario():
    inp = S.inputs()
    g = np.load(os.path.join(GOLDEN, "frame_rgbd_reference.npz"))
    assert S.inputs_digest(inp) == str(g["inputs_digest"]), "the synthetic inputs changed: regenerate with scripts/make_frame_rgbd_golden.py"
    return inp, {k: g[k] for k in g.files}


# ---------------------------------------------------------------------------------------------------------------- CPU
def test_inputs_digest_matches(scenario):
    inp, g = scenario
    with open(os.path.join(GOLDEN, "frame_rgbd_reference_facts.json")) as f:
        assert json.load(f)["inputs"] == S.inputs_digest(inp) == str(g["inputs_digest"])
    assert inp["depth"].shape == (S.H, S.PITCH) and (inp["depth"][:, S.W:] == S.PAD).all()


def test_restatement_equals_the_reference(scenario):
    inp, g = scenario
    xy = np.stack([inp["kps"]["x"], inp["kps"]["y"]], -1)
    ur, z = R.stereo_from_rgbd(xy, inp["kps_un"]["x"], S.image_of(inp), inp["mbf"])
    assert same(ur, g["u_right"]) and same(z, g["depth"])
    assert same(np.array([R.scene_median_depth(z)]), g["median"])
    counters = {}
    out = R.stereo_lines_from_rgbd(S.lines8(inp), S.image_of(inp), inp["K4"], inp["mbf"], inp["min_line_length_3d"], counters)
    for k, o in zip(LINE_KEYS, out):
        assert same(o, g[k]), k
    with open(os.path.join(GOLDEN, "frame_rgbd_reference_facts.json")) as f:
        facts = json.load(f)["facts"]
    assert {k: facts[k] for k in R.BRANCHES} == counters


def test_the_golden_run_takes_every_branch():
    with open(os.path.join(GOLDEN, "frame_rgbd_reference_facts.json")) as f:
        facts = json.load(f)["facts"]
    for k in ("misaligned", "repaired_emax", "repaired_smax", "rejected", "short", "view_angle", "no_middle", "no_end_point"):
        assert facts[k] >= 5, (k, facts[k])
    assert facts["stereo"] >= 150
    assert facts["points_without_depth"] >= 20 and facts["points_inf"] >= 3


def test_header_declares_and_library_exports_the_entries():
    with open(os.path.join(ROOT, "include", "plvs_hip.h")) as f:
        header = f.read()
    assert "Frame glue, RGB-D" in header
    from plvs_amd import _lib      # (loads the library the way the package does: after torch, one HIP runtime per process)
    assert os.path.samefile(_lib.LIB_PATH, os.path.join(ROOT, "plvs_amd", "lib", "libplvs_hip.so"))
    lib = _lib.lib
    for name in ENTRIES:
        assert re.search(r"\bint " + name + r"\(", header), f"{name} is not declared in include/plvs_hip.h"
        assert hasattr(lib, name), f"libplvs_hip.so does not export {name}"
    lib.plvs_hip_abi_version.restype = ctypes.c_int
    assert lib.plvs_hip_abi_version() == 1


# ---------------------------------------------------------------------------------------------------------------- GPU
def _golden_points(g):
    return g["u_right"], g["depth"]


def _golden_lines(g):
    return tuple(g[k] for k in LINE_KEYS)


def _check(got, want):
    assert len(got) == len(want)
    for a, b in zip(got, want):
        assert same(a, b)


@pytest.mark.gpu
def test_host_flavours_equal_the_reference(scenario):
    from plvs_amd import frame
    from plvs_amd.lines import KEYLINE_DTYPE
    from plvs_amd.orb import KP_DTYPE
    assert KP_DTYPE == S.KP_DTYPE and KEYLINE_DTYPE == S.KEYLINE_DTYPE
    inp, g = scenario
    _check(frame.ComputeStereoFromRGBD(inp["kps"], inp["kps_un"], S.image_of(inp), inp["mbf"]), _golden_points(g))   # pitched view
    _check(frame.ComputeStereoLinesFromRGBD(inp["keylines"], inp["keylines_un"], S.image_of(inp), inp["K4"], inp["mbf"],
                                            inp["min_line_length_3d"]), _golden_lines(g))
    tight = np.ascontiguousarray(S.image_of(inp))
    _check(frame.ComputeStereoFromRGBD(inp["kps"], inp["kps_un"], tight, inp["mbf"]), _golden_points(g))


@pytest.mark.gpu
def test_device_flavour_equals_the_reference(scenario):
    import torch
    from plvs_amd import frame
    inp, g = scenario
    pitched = torch.from_numpy(inp["depth"]).cuda()[:, :S.W]
    tight = torch.from_numpy(np.ascontiguousarray(S.image_of(inp))).cuda()
    assert pitched.stride(0) == S.PITCH and tight.stride(0) == S.W
    args = (inp["K4"], inp["mbf"], inp["min_line_length_3d"])
    want = _golden_points(g) + _golden_lines(g)
    for d in (pitched, tight):
        _check(frame.stereo_from_rgbd(inp["kps"], inp["kps_un"], inp["keylines"], inp["keylines_un"], d, *args), want)
    # either count zero, and one of each (the middle of the arrays)
    _check(frame.stereo_from_rgbd(inp["kps"][:0], inp["kps_un"][:0], inp["keylines"], inp["keylines_un"], pitched, *args),
           tuple(w[:0] for w in want[:2]) + want[2:])
    _check(frame.stereo_from_rgbd(inp["kps"], inp["kps_un"], inp["keylines"][:0], inp["keylines_un"][:0], pitched, *args),
           want[:2] + tuple(w[:0] for w in want[2:]))
    _check(frame.stereo_from_rgbd(inp["kps"][:0], inp["kps_un"][:0], inp["keylines"][:0], inp["keylines_un"][:0], pitched, *args),
           tuple(w[:0] for w in want))
    stereo = int(np.flatnonzero(g["depth_start"] > 0)[3])
    withd = int(np.flatnonzero(g["depth"] > 0)[3])
    _check(frame.stereo_from_rgbd(inp["kps"][withd:withd + 1], inp["kps_un"][withd:withd + 1], inp["keylines"][stereo:stereo + 1],
                                  inp["keylines_un"][stereo:stereo + 1], pitched, *args),
           tuple(w[withd:withd + 1] for w in want[:2]) + tuple(w[stereo:stereo + 1] for w in want[2:]))
    # the mirrors of the two reference functions take the device image too
    _check(frame.ComputeStereoFromRGBD(inp["kps"], inp["kps_un"], pitched, inp["mbf"]), want[:2])
    _check(frame.ComputeStereoLinesFromRGBD(inp["keylines"], inp["keylines_un"], pitched, *args), want[2:])


@pytest.mark.gpu
def test_key_points_outside_the_image_get_minus_one(scenario):
    import torch
    from plvs_amd import frame
    inp, _ = scenario
    image = S.image_of(inp).copy()
    image[:] = 2.0
    xy = np.array([[-3.0, 5.0], [S.W, 5.0], [5.0, -1.0], [5.0, S.H], [1e9, 5.0], [5.0, -1e9], [-1.0, -1.0], [3e38, 3e38],
                   [-0.5, 5.0], [S.W - 0.25, S.H - 0.25], [5.0, 5.0]], np.float32)     # the last three: inside (truncation)
    kps = np.zeros(len(xy), S.KP_DTYPE)
    kps["x"], kps["y"] = xy[:, 0], xy[:, 1]
    want_z = np.array([-1] * 8 + [2] * 3, np.float32)
    want_u = np.where(want_z > 0, kps["x"] - inp["mbf"] / np.float32(2.0), np.float32(-1)).astype(np.float32)
    for d in (image, torch.from_numpy(image).cuda()):
        _check(frame.ComputeStereoFromRGBD(kps, kps, d, inp["mbf"]), (want_u, want_z))


@pytest.mark.gpu
def test_scene_median_depth(scenario):
    from plvs_amd import frame
    _, g = scenario
    assert same(np.array([frame.ComputeSceneMedianDepth(g["depth"])]), g["median"])
    assert frame.ComputeSceneMedianDepth(np.array([-1, -1, 0, np.nan], np.float32)) == np.float32(1.5)
    assert frame.ComputeSceneMedianDepth(np.zeros(0, np.float32), 2.25) == np.float32(2.25)
    assert frame.ComputeSceneMedianDepth(np.array([3, -1, np.inf, 1], np.float32)) == np.float32(3)
    assert frame.ComputeSceneMedianDepth(np.array([4, 3, 2, 1], np.float32)) == np.float32(2)


@pytest.mark.gpu
def test_bad_arguments_are_refused(scenario):
    import torch
    from plvs_amd import _lib, frame   # noqa: F401  (frame sets the argtypes)
    L = _lib.lib
    inp, _ = scenario
    n, nl = len(inp["kps"]), len(inp["keylines"])
    depth = np.ascontiguousarray(inp["depth"])
    d_depth = torch.from_numpy(depth).cuda()
    p = _lib.np_ptr
    o = [np.zeros(max(n, nl), np.float32) for _ in range(6)]
    pts = lambda **kw: L.plvs_hip_frame_compute_stereo_from_rgbd(                                       # noqa: E731
        kw.get("kps", p(inp["kps"])), p(inp["kps_un"]), kw.get("n", n), kw.get("depth", p(depth)), kw.get("w", S.W), kw.get("h", S.H),
        kw.get("pitch", S.PITCH), 4.0, kw.get("out", p(o[0])), p(o[1]))
    lns = lambda **kw: L.plvs_hip_frame_compute_stereo_lines_from_rgbd(                                 # noqa: E731
        p(inp["keylines"]), kw.get("klu", p(inp["keylines_un"])), kw.get("n", nl), kw.get("depth", p(depth)), S.W, S.H,
        kw.get("pitch", S.PITCH), kw.get("K4", p(inp["K4"])), 4.0, 0.01, p(o[2]), p(o[3]), p(o[4]), kw.get("out", p(o[5])))
    dev = lambda **kw: L.plvs_hip_frame_stereo_from_rgbd_dev(                                           # noqa: E731
        p(inp["kps"]), kw.get("kps_un", p(inp["kps_un"])), kw.get("n", n), p(inp["keylines"]), p(inp["keylines_un"]), kw.get("nl", nl),
        kw.get("depth", ctypes.c_void_p(d_depth.data_ptr())), kw.get("w", S.W), S.H, kw.get("pitch", S.PITCH), kw.get("K4", p(inp["K4"])),
        4.0, 0.01, p(o[0]), p(o[1]), p(o[2]), p(o[3]), kw.get("out", p(o[4])), p(o[5]), None)
    assert pts() == lns() == dev() == _lib.PLVS_OK
    bad = [pts(n=-1), pts(pitch=S.W - 1), pts(depth=None), pts(kps=None), pts(out=None), pts(w=0), pts(h=-2),
           lns(n=-1), lns(pitch=S.W - 1), lns(depth=None), lns(klu=None), lns(K4=None), lns(out=None),
           dev(n=-1), dev(nl=-1), dev(pitch=S.W - 1), dev(depth=None), dev(kps_un=None), dev(K4=None), dev(out=None), dev(w=0),
           L.plvs_hip_frame_scene_median_depth(p(o[0]), -1, 1.5, p(o[1])), L.plvs_hip_frame_scene_median_depth(None, 3, 1.5, p(o[1])),
           L.plvs_hip_frame_scene_median_depth(p(o[0]), 3, 1.5, None)]
    assert bad == [_lib.PLVS_ERR_INVALID_ARG] * len(bad)
    c, f = frame.RgbdCalib(), frame.RgbdFrameC()
    img = torch.zeros((S.H, S.W), dtype=torch.uint8, device="cuda")
    one = lambda orb, image, w, pitch, calib, fr: L.plvs_hip_frame_rgbd_dev(                             # noqa: E731
        orb, None, image, w, S.H, S.W, ctypes.c_void_p(d_depth.data_ptr()), pitch, calib, fr, None)
    from plvs_amd.orb import ORBextractor
    orb = ORBextractor(500, 1.2, 8, 20, 7)
    ip = ctypes.c_void_p(img.data_ptr())
    bad = [one(None, ip, S.W, S.PITCH, ctypes.byref(c), ctypes.byref(f)), one(orb._h, None, S.W, S.PITCH, ctypes.byref(c), ctypes.byref(f)),
           one(orb._h, ip, S.W, S.W - 1, ctypes.byref(c), ctypes.byref(f)), one(orb._h, ip, S.W, S.PITCH, None, ctypes.byref(f)),
           one(orb._h, ip, S.W, S.PITCH, ctypes.byref(c), None),
           one(orb._h, ip, S.W, S.PITCH, ctypes.byref(c), ctypes.byref(f))]      # (no output arrays, capacity 0)
    assert bad == [_lib.PLVS_ERR_INVALID_ARG] * len(bad)


# ---- the constructor in one call against the separate entries in the constructor's order
TUM1_K = (517.3, 516.5, 318.6, 255.3)
TUM1_D = (0.2624, -0.9531, -0.0054, 0.0026, 1.1633)
MBF = 40.0


def _synthetic_depth(h, w, pitch):
    rng = np.random.default_rng(5)
    x, y = np.meshgrid(np.arange(w, dtype=np.float32), np.arange(h, dtype=np.float32))
    d = np.full((h, pitch), -7.0, np.float32)
    img = (np.float32(1.2) + np.float32(0.003) * x + np.float32(0.001) * y).astype(np.float32)     # a plane
    img[140:330, 220:430] = np.float32(0.8)                                                        # a box in front of it
    img[60:100, 500:560] = 0.0                                                                     # holes
    img[400:430, 80:140] = 0.0
    img[rng.random((h, w)) < 0.03] = np.nan
    d[:, :w] = img
    return d


def _separate(orb, lines, image, depth, bounds4, gw, gh, use_median):
    """The entries one by one, in the order of src/Frame.cc:498-580."""
    from plvs_amd import frame
    if lines is not None:
        mono, kps, desc, kl, kld = frame.extract_frame(orb, lines, image)
    else:
        mono, kps, desc = orb(image)
        kl, kld = np.zeros(0, S.KEYLINE_DTYPE), np.zeros((0, 32), np.uint8)
    un = frame.UndistortKeyPoints(kps, TUM1_K, TUM1_D)
    ur, z = frame.ComputeStereoFromRGBD(kps, un, depth, MBF)
    out = dict(mono_index=mono, keys=kps, keys_un=un, descriptors=desc, u_right=ur, depth=z,
               median_depth=frame.ComputeSceneMedianDepth(z) if use_median else np.float32(1.5))
    n_extracted = len(kl)
    if len(kl):
        klu, kept = frame.UndistortKeyLines(kl, TUM1_K, TUM1_D, bounds4)
        kl, kld = kl[kept], kld[kept]
        ls = frame.ComputeStereoLinesFromRGBD(kl, klu, depth, TUM1_K, MBF)
    else:
        klu, ls = kl, tuple(np.zeros(0, np.float32) for _ in range(4))
    out.update(keylines=kl, keylines_un=klu, line_descriptors=kld, **dict(zip(LINE_KEYS, ls)))
    out["cell_start"], out["cell_items"] = frame.AssignFeaturesToGrid(un, bounds4[0], bounds4[2], gw, gh)
    return out, n_extracted


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
    from tests.oracle_lib import golden
    grey = golden("aloe_640x480.pgm")
    h, w = grey.shape
    assert (h, w) == (480, 640)
    image = torch.from_numpy(grey).cuda()
    depth = torch.from_numpy(_synthetic_depth(h, w, 704)).cuda()[:, :w]
    b = frame.ComputeImageBounds(w, h, TUM1_K, TUM1_D)
    gw, gh = np.float32(64) / (np.float32(b[1]) - np.float32(b[0])), np.float32(48) / (np.float32(b[3]) - np.float32(b[2]))
    bounds4 = (b[0], b[1] - 60.0, b[2], b[3])      # the caller's bounds: narrower on the right, so that lines are dropped
    orb, lines = ORBextractor(1000, 1.2, 8, 20, 7), LineExtractor(100)
    kw = dict(K=TUM1_K, dist=TUM1_D, mbf=MBF, bounds=bounds4, grid_w_inv=gw, grid_h_inv=gh)
    for with_lines, use_median in ((True, True), (False, False)):
        ex = lines if with_lines else None
        want, n_extracted = _separate(orb, ex, image, depth, bounds4, gw, gh, use_median)
        got = frame.rgbd_frame(orb, ex, image, depth, use_median_depth=use_median, **kw)
        _same_frame(got, want)
        assert len(got["keys"]) > 500 and (got["depth"] > 0).sum() > 300 and (got["depth"] < 0).sum() > 10
        assert got["cell_start"][-1] == len(got["cell_items"]) > 500
        if with_lines:
            assert 20 < len(got["keylines"]) < n_extracted, "no line was dropped: the compaction is not exercised"
            assert (got["depth_start"] > 0).sum() > 10 and (got["depth_start"] < 0).sum() > 0
            assert got["median_depth"] != np.float32(1.5)
        else:
            assert len(got["keylines"]) == len(got["line_descriptors"]) == len(got["depth_end"]) == 0
            assert got["median_depth"] == np.float32(1.5)
    # no key points: zero counts, PLVS_OK, before the lines are touched
    blank = torch.zeros((h, w), dtype=torch.uint8, device="cuda")
    got = frame.rgbd_frame(orb, lines, blank, depth, use_median_depth=True, **kw)
    for k in ("keys", "keys_un", "descriptors", "u_right", "depth", "keylines", "keylines_un", "line_descriptors", "cell_items") + LINE_KEYS:
        assert len(got[k]) == 0, k
    assert not got["cell_start"].any() and got["median_depth"] == np.float32(1.5)
