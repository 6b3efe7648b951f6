"""libelas' host stages on the device and Elas::process in one call (plvs_hip_elas_support_points / _disparity_planes /
_create_grid / _process) against the reference pipeline compiled from its own sources (oracle/_ref/libelas_ref.so,
tests/elas_ref.py): the support list its filters and corners leave, the planes and grids it hands to computeDisparity,
and the final maps of Elas::process."""
import numpy as np
import pytest

from tests import elas_ref
from tests.test_elas_delaunay import MIDDLEBURY, ROBOTICS, fuzz_grid, pair

needs_ref = pytest.mark.skipif(not elas_ref.available(), reason="needs oracle/_ref/libelas_ref.so (built where /root/reference is)")
PLANES = ("t1a", "t1b", "t1c", "t2a", "t2b", "t2c")


def elas(subsampling=False, setting=ROBOTICS):
    from plvs_amd.elas import ElasGPU
    return ElasGPU(ElasGPU.Parameters(subsampling=subsampling, add_corners=setting == MIDDLEBURY))


def reference_support(left, right, grid, subsampling, setting):
    """The support list the reference's filters and corners make of an injected candidate grid."""
    seen = []

    def record(a):
        seen.append(a["support"])
        return np.zeros(a["height"] // 2 * (a["width"] // 2) if a["subsampling"] else a["height"] * a["width"], np.float32)
    elas_ref.run_with(left, right, record, None, subsampling=subsampling, plvs=setting, support_candidates=lambda a: grid)
    return seen[0] if seen else None


@pytest.mark.gpu
@needs_ref
@pytest.mark.parametrize("subsampling", [False, True])
@pytest.mark.parametrize("setting", [ROBOTICS, MIDDLEBURY])
def test_support_points_of_the_device_candidate_grid(subsampling, setting):
    left, right = pair("urban1")
    e = elas(subsampling, setting)
    e.setImages(left, right)
    h, w = left.shape
    grid = e.supportCandidates(None, None, w, h)
    want = reference_support(left, right, grid, subsampling, setting)
    got = e.supportPoints(grid, w, h)
    assert np.array_equal(got.view(np.int32), want.view(np.int32))
    e.supportCandidates(None, None, w, h)                    # the grid left in HBM
    assert np.array_equal(e.supportPoints(None, w, h).view(np.int32), want.view(np.int32))


@pytest.mark.gpu
@needs_ref
def test_support_points_of_fuzzed_candidate_grids():
    left, right = pair("urban1_333")
    h, w = left.shape
    es = {}
    for seed in range(60):
        subsampling, setting = bool(seed % 4 == 3), MIDDLEBURY if seed % 2 else ROBOTICS
        e = es.setdefault((subsampling, setting), elas(subsampling, setting))
        cw, ch, _ = e.candidateGrid(w, h)
        grid = fuzz_grid(seed, (ch, cw))
        want = reference_support(left, right, grid, subsampling, setting)
        got = e.supportPoints(grid, w, h)
        if want is None:                                     # (fewer than 3: the reference stops before computeDisparity)
            assert len(got) < 3, seed
        else:
            assert np.array_equal(got.view(np.int32), want.view(np.int32)), seed


@pytest.mark.gpu
@needs_ref
@pytest.mark.parametrize("name", ["urban1", "urban1_333", "cones"])
@pytest.mark.parametrize("subsampling", [False, True])
@pytest.mark.parametrize("setting", [ROBOTICS, MIDDLEBURY])
def test_planes_and_grids_of_captured_calls(name, subsampling, setting):
    left, right = pair(name)
    calls, _, _ = elas_ref.capture(left, right, subsampling=subsampling, plvs=setting)
    e = elas(subsampling, setting)
    for c in calls:
        bare = c["tri"].copy()
        for k in PLANES:
            bare[k] = 0
        got = e.computeDisparityPlanes(c["support"], bare)
        for k in PLANES:
            assert np.array_equal(got[k].view(np.uint32), c["tri"][k].view(np.uint32)), k
        grid, dims = e.createGrid(c["support"], c["width"], c["height"], c["right_image"])
        assert np.array_equal(dims, c["grid_dims"])
        assert np.array_equal(grid, c["grid"])


@pytest.mark.gpu
def test_singular_planes_are_zero():
    from plvs_amd.elas import SUPPORT_PT, TRIANGLE
    s = np.zeros(4, SUPPORT_PT)
    s["u"], s["v"], s["d"] = [0, 10, 20, 10], [0, 10, 20, 0], [1, 2, 3, 4]   # 0, 1, 2 collinear
    t = np.zeros(3, TRIANGLE)
    t["c1"], t["c2"], t["c3"] = [0, 0, 0], [1, 0, 1], [2, 1, 3]
    got = elas().computeDisparityPlanes(s, t)
    for k in PLANES:
        assert got[k][1] == 0                                # two equal corners: singular
    assert got["t1a"][2] != 0 or got["t1b"][2] != 0


SIZES = ["urban1", "urban1_640", "urban1_333", "cones", "aloe"]


@pytest.mark.gpu
@needs_ref
@pytest.mark.parametrize("name", SIZES)
@pytest.mark.parametrize("subsampling", [False, True])
@pytest.mark.parametrize("only_left", [True, False])
def test_process_equals_the_reference(name, subsampling, only_left):
    left, right = pair(name)
    want = elas_ref.reference(left, right, subsampling=subsampling, plvs=1 if only_left else 0)
    got = elas(subsampling).process(left, right, postprocess_only_left=only_left)
    for g, w in zip(got, want):
        assert np.array_equal(g.view(np.uint32), w.view(np.uint32))
    assert (want[0] >= 0).mean() > 0.2


@pytest.mark.gpu
@needs_ref
@pytest.mark.parametrize("subsampling", [False, True])
def test_process_without_download_feeds_depth_like_the_stage_chain(subsampling):
    import torch
    left, right = pair("urban1")
    h, w = left.shape
    e = elas(subsampling)
    assert e.process(left, right, download=False) is None
    a = torch.zeros((h, w), dtype=torch.float32, device="cuda")
    e.depthDev(400.0, 2, a)
    torch.cuda.synchronize()
    calls, _, _ = elas_ref.capture(left, right, subsampling=subsampling, plvs=1)
    f = elas(subsampling)
    for c in calls:
        f.computeDisparity(c["support"], c["tri"], c["grid"], c["grid_dims"], c["I1_desc"], c["I2_desc"], c["right_image"], w, h,
                           download=False)
    f.postProcess(w, h, download=False)
    b = torch.zeros((h, w), dtype=torch.float32, device="cuda")
    f.depthDev(400.0, 2, b)
    torch.cuda.synchronize()
    assert torch.equal(a.view(torch.int32), b.view(torch.int32))


@pytest.mark.gpu
@needs_ref
def test_one_handle_over_changing_sizes():
    e = elas(False)
    for name in ("urban1", "urban1_333", "urban1"):
        left, right = pair(name)
        want = elas_ref.reference(left, right, subsampling=False, plvs=1)
        for g, w in zip(e.process(left, right), want):
            assert np.array_equal(g.view(np.uint32), w.view(np.uint32)), name


@pytest.mark.gpu
def test_process_errors():
    import ctypes
    from plvs_amd import _lib
    e = elas(False)
    flat = np.full((64, 80), 128, np.uint8)                  # textureless: no support point
    D1 = np.full((64, 80), 7.0, np.float32)
    D2 = D1.copy()
    dims = np.array([80, 64, 80], np.int32)
    rc = _lib.lib.plvs_hip_elas_process(e._h, _lib.np_ptr(flat), _lib.np_ptr(flat), _lib.np_ptr(dims), 1, 1, _lib.np_ptr(D1),
                                        _lib.np_ptr(D2))
    assert rc == _lib.PLVS_ERR_EMPTY and (D1 == 7.0).all() and (D2 == 7.0).all()
    left, right = pair("urban1_333")
    h, w = left.shape
    e.setImages(left, right)
    grid = e.supportCandidates(None, None, w, h)
    n_all = len(e.supportPoints(grid, w, h))
    with pytest.raises(_lib.PlvsHipError) as err:
        e.supportPoints(grid, w, h, cap=n_all - 1)
    assert err.value.code == _lib.PLVS_ERR_CAPACITY
    n = ctypes.c_int()
    out = np.zeros(3, np.int32)
    assert _lib.lib.plvs_hip_elas_support_points(e._h, _lib.np_ptr(grid), w, h, _lib.np_ptr(out), 1, ctypes.byref(n)) == \
        _lib.PLVS_ERR_CAPACITY and n.value == n_all
    with pytest.raises(_lib.PlvsHipError) as err:           # 40 x 40 at grid 20: 2 x 2 cells < 2 * 2 + 2
        e.createGrid(np.zeros(3, e.supportPoints(grid, w, h).dtype), 40, 40, 0)
    assert err.value.code == _lib.PLVS_ERR_INVALID_ARG
    for bad in ([8, 64, 80], [80, 64, 40]):
        dims = np.array(bad, np.int32)
        assert _lib.lib.plvs_hip_elas_process(e._h, _lib.np_ptr(flat), _lib.np_ptr(flat), _lib.np_ptr(dims), 1, 1, None,
                                              None) == _lib.PLVS_ERR_INVALID_ARG
