"""The HIP stages of libelas' post-processing and computeDisparity's triangle loop against the oracle on the synthetic cases
of tests/elas_synth.py (the oracle itself is held to the compiled reference on them by tests/test_elas_synth_reference.py):
segments at the speckle size and at the similarity threshold, shapes that stress the run / link split of the union-find,
widths around seg_rows' chunking, gaps of exactly the gap width and one more, lines without valid pixels, windows of
adaptiveMean that do not fit, disparities that warp to the map's edges, and triangle lists whose ORDER decides the map.
Every comparison is bit for bit.  Every map is a few hundred pixels wide at most."""
import numpy as np
import pytest

from tests import elas_synth
from tests.test_elas import golden_capture

pytestmark = pytest.mark.gpu

MAP_CASES = elas_synth.map_cases()
BY_NAME = {c["name"]: c for c in MAP_CASES}
_HANDLES = {}


def handle(**params):
    """One handle per parameter set for the whole module: the cases that share it change size from call to call, growing
    and shrinking, so the handle's reserved buffers (and the zeroing of seg_rows' run lengths) are reused across sizes."""
    from plvs_amd.elas import ElasGPU
    key = tuple(sorted(params.items()))
    if key not in _HANDLES:
        _HANDLES[key] = ElasGPU(ElasGPU.Parameters(**params))
    return _HANDLES[key]


def bit_equal(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def differing(a, b):
    return int((a.view(np.uint32) != b.view(np.uint32)).sum())


def stage_params(case):
    p = dict(subsampling=case["subsampling"])
    if case["stage"] == "seg":
        p.update(speckle_size=case["speckle_size"], speckle_sim_threshold=elas_synth.SIM)
    elif case["stage"] == "gap":
        p.update(ipol_gap_width=case["ipol_gap_width"], add_corners=case["add_corners"])
    elif case["stage"] == "lr":
        p.update(lr_threshold=case["lr_threshold"])
    return p


def device_stage(e, case):
    w, h = case["width"], case["height"]
    if case["stage"] == "seg":
        return [e.removeSmallSegments(case["D"], w, h)]
    if case["stage"] == "gap":
        return [e.gapInterpolation(case["D"], w, h)]
    if case["stage"] == "mean":
        return [e.adaptiveMean(case["D"], w, h).reshape(case["D"].shape)]
    return list(e.leftRightConsistencyCheck(case["D1"], case["D2"], w, h))


def oracle_stage(oracle, case):
    sub = case["subsampling"]
    if case["stage"] == "lr":
        A, B = case["D1"].copy(), case["D2"].copy()
        oracle.elas_left_right_check(A, B, sub, case["lr_threshold"])
        return [A, B]
    D = case["D"].copy()
    if case["stage"] == "seg":
        oracle.elas_remove_small_segments(D, sub, case["speckle_size"], elas_synth.SIM)
    elif case["stage"] == "gap":
        oracle.elas_gap_interpolation(D, sub, case["ipol_gap_width"], case["add_corners"])
    else:
        D = oracle.elas_adaptive_mean(D, case["width"], case["height"], sub)
    return [D]


@pytest.mark.parametrize("name", list(BY_NAME))
def test_stage_equals_the_oracle(oracle, name):
    case = BY_NAME[name]
    elas_synth.assert_facts(case)
    got, want = device_stage(handle(**stage_params(case)), case), oracle_stage(oracle, case)
    for k, (g, w) in enumerate(zip(got, want)):
        assert bit_equal(g, w), f"{name} map {k + 1}: {differing(g, w)} of {g.size} pixels differ"


def test_one_handle_across_every_stage_and_size(oracle):
    """One handle, all four stages, the maps' sizes going up and down between calls (2 x 2 ... 257 x 60 ... 2 x 60): every
    stage shares the handle's scratch buffers with the others, and a small map follows a large one whose run lengths,
    parents and sizes still lie behind it in the same buffers."""
    from plvs_amd.elas import ElasGPU
    e = ElasGPU(ElasGPU.Parameters(speckle_size=12, ipol_gap_width=3, lr_threshold=2))
    mine = [c for c in MAP_CASES if not c["subsampling"] and c.get("speckle_size", 12) == 12 and c.get("ipol_gap_width", 3) == 3
            and not c.get("add_corners") and c.get("lr_threshold", 2) == 2]
    small = sorted(mine, key=lambda c: c["width"] * c["height"])
    order = [c for pair_ in zip(small[:len(small) // 2], reversed(small)) for c in pair_]      # small, large, small, large ...
    assert {c["stage"] for c in order} == {"seg", "gap", "mean", "lr"} and len(order) > 30
    sizes = [c["width"] * c["height"] for c in order]
    assert min(sizes) == 4 and max(sizes) > 15000 and any(a > 50 * b for a, b in zip(sizes, sizes[1:]))
    for rep in range(2):
        for c in order:
            for g, w in zip(device_stage(e, c), oracle_stage(oracle, c)):
                assert bit_equal(g, w), f"{c['name']} (round {rep}): {differing(g, w)} pixels differ"
    e.close()


@pytest.mark.parametrize("subsampling", [False, True])
def test_chain_of_stand_alone_calls_equals_the_oracles_chain(oracle, subsampling):
    """lr -> seg -> gap -> mean on a pair that holds -1, -10, speckles and holes: the left/right check is what brings the maps
    inside removeSmallSegments' precondition."""
    case = elas_synth.chain_case(subsampling)
    elas_synth.assert_facts(case)
    w, h = case["width"], case["height"]
    e = handle(subsampling=subsampling, speckle_size=12, lr_threshold=2, ipol_gap_width=3)
    want = [case["D1"].copy(), case["D2"].copy()]
    assert (want[0] == -1).any() and (want[1] == -1).any()
    got = list(e.leftRightConsistencyCheck(want[0], want[1], w, h))
    oracle.elas_left_right_check(want[0], want[1], subsampling, 2)
    steps = ["lr"]
    for k in range(2):
        assert bit_equal(got[k], want[k]), ("lr", k)
        assert not (want[k] == -1).any() and (want[k] >= 0).sum() > 1000
        before = want[k].copy()
        got[k] = e.removeSmallSegments(got[k], w, h)
        oracle.elas_remove_small_segments(want[k], subsampling, 12, elas_synth.SIM)
        assert bit_equal(got[k], want[k]) and not bit_equal(want[k], before), ("seg", k)
        before = want[k].copy()
        got[k] = e.gapInterpolation(got[k], w, h)
        oracle.elas_gap_interpolation(want[k], subsampling, 3, False)
        assert bit_equal(got[k], want[k]) and not bit_equal(want[k], before), ("gap", k)
        before = want[k].copy()
        got[k] = e.adaptiveMean(got[k], w, h).reshape(before.shape)
        want[k] = oracle.elas_adaptive_mean(want[k], w, h, subsampling)
        assert bit_equal(got[k], want[k]) and not bit_equal(want[k], before), ("mean", k)
        steps += ["seg", "gap", "mean"]
    assert len(steps) == 7


# ------------------------------------------------------------------ computeDisparity: the last triangle over a pixel wins
def _disparity(e, a):
    return e.computeDisparity(a["support"], a["tri"], a["grid"], a["grid_dims"], a["I1_desc"], a["I2_desc"], a["right_image"],
                              a["width"], a["height"])


@pytest.mark.parametrize("setting", elas_synth.TRI_SETTINGS, ids=lambda s: f"sub{s['subsampling']}_texture{s['match_texture']}")
def test_triangle_lists_equal_the_oracle_in_their_order(oracle, setting):
    """Shuffled, appended, reversed, prepended and degenerate triangle lists on the committed capture, left and right image.
    The two orders of the overlapping list must give two different maps, each equal to the oracle's for that order: a device
    that let the first triangle win, or any fixed one, fails here."""
    calls, _ = golden_capture()
    e = handle(subsampling=bool(setting["subsampling"]), match_texture=setting["match_texture"])
    maps = {}
    for case in elas_synth.triangle_cases(calls):
        elas_synth.assert_facts(case)
        for a in case["calls"]:
            a = dict(a, subsampling=setting["subsampling"])
            got = _disparity(e, a)
            want = oracle.elas_compute_disparity(a, match_texture=setting["match_texture"])
            assert bit_equal(got, want), f"{case['name']} right_image={a['right_image']}: {differing(got, want)} pixels differ"
            maps[case["name"], a["right_image"]] = got
    for right in (0, 1):
        assert bit_equal(maps["tri_capture_shuffled", right], maps["tri_capture", right])
        if setting["match_texture"] == 10000:
            assert (maps["tri_appended", right] == elas_synth.INVALID).all()
        else:
            scale = 4 if setting["subsampling"] else 1
            assert differing(maps["tri_appended", right], maps["tri_appended_reversed", right]) > 500 // scale
            assert differing(maps["tri_appended", right], maps["tri_prepended", right]) > 500 // scale
            assert (maps["tri_appended", right] >= 0).sum() > 1000 // scale


# ------------------------------------------------------------------ postProcess without the left/right check
def _capture_maps_in_hbm(e):
    calls, _ = golden_capture()
    maps = [_disparity(e, a) for a in calls]
    assert all((m == -10).any() and (m >= 0).any() for m in maps)
    return calls[0]["width"], calls[0]["height"], maps


def test_postprocess_refuses_speckle_removal_without_the_left_right_check():
    from plvs_amd import _lib
    from plvs_amd.elas import ElasGPU
    e = ElasGPU(ElasGPU.Parameters(lr_threshold=-1, speckle_size=200))
    w, h, _ = _capture_maps_in_hbm(e)
    with pytest.raises(_lib.PlvsHipError, match="lr_threshold < 0") as err:
        e.postProcess(w, h)
    assert err.value.code == _lib.PLVS_ERR_INVALID_ARG
    with pytest.raises(_lib.PlvsHipError, match="lr_threshold < 0") as err:       # Elas::process in one call: before any work
        e.process(np.zeros((64, 64), np.uint8), np.zeros((64, 64), np.uint8))
    assert err.value.code == _lib.PLVS_ERR_INVALID_ARG
    e.close()


@pytest.mark.parametrize("only_left", [True, False])
def test_postprocess_without_check_and_speckles_equals_the_oracles_gaps_and_mean(oracle, only_left):
    from plvs_amd.elas import ElasGPU
    e = ElasGPU(ElasGPU.Parameters(lr_threshold=-1, speckle_size=0))
    w, h, maps = _capture_maps_in_hbm(e)
    got = e.postProcess(w, h, postprocess_only_left=only_left)
    want = [m.copy() for m in maps]
    for k in range(1 if only_left else 2):
        oracle.elas_gap_interpolation(want[k], False, 3, False)
        want[k] = oracle.elas_adaptive_mean(want[k], w, h, False)
    for k in range(2):
        assert bit_equal(got[k], want[k]), f"map {k + 1}: {differing(got[k], want[k])} pixels differ"
    assert not bit_equal(got[0], maps[0]) and (bit_equal(got[1], maps[1]) == only_left)
    e.close()
