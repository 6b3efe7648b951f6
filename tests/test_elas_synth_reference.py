"""The oracle's libelas post-processing held to the COMPILED reference on the synthetic cases of tests/elas_synth.py (CPU).

A map reaches the reference's own removeSmallSegments / gapInterpolation / leftRightConsistencyCheck through the hooks of
tests/elas_ref.py: the reference pipeline runs on a crop of urban1 cut to the case's size, a hook in front of the stage
overwrites both maps (the case in D1, the case turned by 180 degrees in D2: both maps of a run carry a case), the stage
itself stays the reference's compiled code, and a recording hook behind it reads the result.  The parameters are the
reference's two sets (ROBOTICS, mode 0; MIDDLEBURY, mode 2: elas.h:97-155), so only cases with those parameters get there
(speckle_size 200, lr_threshold 2, gaps of 3 or of 5000 with add_corners); adaptiveMean is called directly.

Which sizes are NOT injected: the pipeline needs three support points and a disparity grid of three rows before it reaches
post-processing — crops below 97 x 60 pixels return early or do not survive createGrid.  Cases on smaller images (every map
of H or W below 30, mean maps of fewer rows than the reference loads ahead: 7, or 3 with subsampling) are held to the oracle's own invariants instead
(test_small_cases_hold_the_oracles_invariants).  Where oracle/_ref is absent the recorded digests of the reference's results
(tests/golden/elas_synth_reference_digests.json, scripts/make_elas_synth_golden.py) stand in.

The triangle cases: the reference's computeDisparity can only be called with the pipeline's own arguments (tests/test_elas.py
pins the oracle's there); what is asserted here, on the oracle, is that the cases DO depend on the triangle order."""
import ctypes
import hashlib
import json
import os

import numpy as np
import pytest

from tests import elas_ref, elas_synth
from tests.test_elas import GOLDEN, golden_capture, pair

needs_ref = pytest.mark.skipif(not elas_ref.available(), reason="needs oracle/_ref/libelas_ref.so (the compiled reference)")
DIGESTS = os.path.join(GOLDEN, "elas_synth_reference_digests.json")
REF_MIN_WIDTH, REF_MIN_HEIGHT = 97, 60          # image sizes from which the reference pipeline reaches post-processing
ROBOTICS, MIDDLEBURY = 0, 2                     # (modes of ref_elas_process_hooked; both post-process the right map too)

MAP_CASES = elas_synth.map_cases()
BY_NAME = {c["name"]: c for c in MAP_CASES}
assert len(BY_NAME) == len(MAP_CASES)


def modes(case):
    """The reference parameter sets under which the compiled stage computes what the case asks for."""
    if case["width"] < REF_MIN_WIDTH or case["height"] < REF_MIN_HEIGHT or case["width"] > 1241 or case["height"] > 376:
        return []
    if case["stage"] == "seg":
        return [ROBOTICS, MIDDLEBURY] if case["speckle_size"] == 200 else []
    if case["stage"] == "lr":
        return [ROBOTICS, MIDDLEBURY] if case["lr_threshold"] == 2 else []
    if case["stage"] == "gap":
        return {(3, False): [ROBOTICS], (5000, True): [MIDDLEBURY]}.get((case["ipol_gap_width"], case["add_corners"]), [])
    return []


REACHABLE = [c["name"] for c in MAP_CASES if modes(c)]
SMALL = [c["name"] for c in MAP_CASES if not modes(c) and c["stage"] != "mean"]
# (adaptiveMean is called directly, on maps of any size: the reference is compiled with a zero-filling malloc,
# oracle/ref/elas_zero_malloc.h, so the scratch image it reads without having written it holds zeros whatever its size)
def _mean_rows_preloaded(c):       # the vertical pass of the reference loads taps - 1 rows before it looks at the height
    return c["D"].shape[0] >= (3 if c["subsampling"] else 7)


MEAN_REF = [c["name"] for c in MAP_CASES if c["stage"] == "mean" and _mean_rows_preloaded(c)]
MEAN_SMALL = [c["name"] for c in MAP_CASES if c["stage"] == "mean" and not _mean_rows_preloaded(c)]


def crop(case):
    left, right = pair()
    h, w = left.shape
    x, y = min(330, w - case["width"]), min(170, h - case["height"])
    return (np.ascontiguousarray(left[y:y + case["height"], x:x + case["width"]]),
            np.ascontiguousarray(right[y:y + case["height"], x:x + case["width"]]))


def two_maps(case):
    """What goes into (D1, D2)."""
    if case["stage"] == "lr":
        return case["D1"], case["D2"]
    return case["D"], np.ascontiguousarray(case["D"][::-1, ::-1])


def _inject(case):
    A, B = two_maps(case)

    def lr(D1, D2):
        assert D1.shape == A.shape, (D1.shape, A.shape)
        D1[:], D2[:] = A, B
    return lr


def _nothing(D):
    pass


def reference_results(case, mode, gap_by=None):
    """The compiled reference's stage on the case's two maps -> [result of D1, result of D2].  gap_by: a function in place
    of the reference's gapInterpolation (MIDDLEBURY gap cases only, see test_oracle_equals_the_compiled_reference)."""
    left, right = crop(case)
    sub = case["subsampling"]
    seen = []
    if case["stage"] == "seg":
        elas_ref._run(left, right, sub, mode, None, None, post=dict(left_right_check=_inject(case),
                                                                   gap_interpolation=lambda D: seen.append(D.copy())))
    elif case["stage"] == "lr":
        A, B = two_maps(case)

        def disparity(args, D):
            D[:] = (B if args["right_image"] else A).reshape(-1)
        elas_ref._run(left, right, sub, mode, disparity, None, post=dict(remove_small_segments=lambda D: seen.append(D.copy())))
    elif mode == ROBOTICS:        # gapInterpolation, read where adaptiveMean receives it
        elas_ref._run(left, right, sub, mode, None, lambda args, D: seen.append(D.copy().reshape(case["D"].shape)),
                      post=dict(left_right_check=_inject(case), remove_small_segments=_nothing))
    else:                         # MIDDLEBURY: no adaptive mean; the pipeline's median-filtered result is all that shows
        ran = []
        post = dict(left_right_check=lambda D1, D2: (ran.append(1), _inject(case)(D1, D2)), remove_small_segments=_nothing)
        if gap_by is not None:
            post["gap_interpolation"] = gap_by
        out = elas_ref._run(left, right, sub, mode, None, None, post=post)
        seen = list(out) if ran else []
    assert len(seen) == 2, f"{case['name']}: the reference pipeline did not reach the hook on this crop"
    return seen


def oracle_results(oracle, case):
    """The oracle's stage on the same two maps."""
    A, B = (m.copy() for m in two_maps(case))
    sub = case["subsampling"]
    if case["stage"] == "seg":
        for D in (A, B):
            oracle.elas_remove_small_segments(D, sub, case["speckle_size"], elas_synth.SIM)
    elif case["stage"] == "gap":
        for D in (A, B):
            oracle.elas_gap_interpolation(D, sub, case["ipol_gap_width"], case["add_corners"])
    elif case["stage"] == "lr":
        oracle.elas_left_right_check(A, B, sub, case["lr_threshold"])
    else:
        return [oracle.elas_adaptive_mean(case["D"], case["width"], case["height"], sub)]
    return [A, B]


def digest(a):
    return hashlib.sha256(np.ascontiguousarray(a, np.float32).tobytes()).hexdigest()


def bit_equal(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def reference_mean(case):
    lib = ctypes.CDLL(elas_ref.REF)
    lib.ref_elas_adaptive_mean.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int]
    want = case["D"].copy()
    lib.ref_elas_adaptive_mean(want.ctypes.data, case["width"], case["height"], int(case["subsampling"]))
    return want


# ------------------------------------------------------------------ the cases themselves
@pytest.mark.parametrize("name", list(BY_NAME))
def test_case_holds_its_facts(name):
    elas_synth.assert_facts(BY_NAME[name])


def test_the_case_list_covers_what_it_promises():
    seg = [c for c in MAP_CASES if c["stage"] == "seg"]
    assert {c["D"].shape[1] for c in seg} >= {2, 63, 255, 256, 257, 513}             # around seg_rows' 256 threads
    assert min(c["D"].shape[0] for c in seg) == 2 and max(c["D"].shape[0] for c in seg) >= 130
    assert {(c["speckle_size"], c["subsampling"]) for c in seg} == {(12, False), (12, True), (200, False), (200, True)}
    assert [elas_synth.speckle_of(s, 1) for s in (12, 200)] == [6, 28]
    gap = [c for c in MAP_CASES if c["stage"] == "gap"]
    assert {(c["ipol_gap_width"], c["add_corners"]) for c in gap} >= {(3, False), (3, True), (5000, True), (64, False), (65, False)}
    assert {elas_synth.gap_of(c["ipol_gap_width"], c["subsampling"]) for c in gap} >= {2, 3, 64, 65}
    mean = [c for c in MAP_CASES if c["stage"] == "mean"]
    assert {c["D"].shape for c in mean} >= {(h, w) for h in (2, 6, 7, 8, 9) for w in (2, 6, 7, 8, 9)}
    assert {c["subsampling"] for c in mean} == {False, True}
    # every stage has cases the compiled reference can be asked about, at both resolutions
    for stage in ("seg", "gap", "lr"):
        assert {BY_NAME[n]["subsampling"] for n in REACHABLE if BY_NAME[n]["stage"] == stage} == {False, True}, stage
    assert max(c["width"] for c in MAP_CASES) <= 1026 and max(c.get("D", c.get("D1")).size for c in MAP_CASES) < 40000


# ------------------------------------------------------------------ against the compiled reference
@needs_ref
@pytest.mark.parametrize("name", REACHABLE)
def test_oracle_equals_the_compiled_reference(oracle, name):
    """Bit for bit on both maps of the run, under every reference parameter set that computes the case.  MIDDLEBURY's gap
    cases: that set has no adaptive mean behind gapInterpolation, only the median filter, so what is compared is the
    pipeline's result with the reference's gapInterpolation against the pipeline's result with the oracle's in its place."""
    case = BY_NAME[name]
    for mode in modes(case):
        want = reference_results(case, mode)
        if case["stage"] == "gap" and mode == MIDDLEBURY:
            got = reference_results(case, mode, gap_by=lambda D: oracle.elas_gap_interpolation(D, case["subsampling"], 5000, True))
        else:
            got = oracle_results(oracle, case)
        for k, (g, w) in enumerate(zip(got, want)):
            assert bit_equal(g, w), f"{name} mode {mode} map {k + 1}: {int((g != w).sum())} pixels differ"


@needs_ref
@pytest.mark.parametrize("name", MEAN_REF)
def test_oracle_adaptive_mean_equals_the_compiled_reference(oracle, name):
    case = BY_NAME[name]
    got, want = oracle_results(oracle, case)[0], reference_mean(case)
    assert bit_equal(got, want), f"{int((got != want).sum())} pixels differ"
    if case["untouched"]:
        assert bit_equal(want, case["D"])


def recorded():
    with open(DIGESTS) as f:
        return json.load(f)


def test_oracle_reproduces_the_recorded_digests_of_the_reference(oracle):
    """Runs everywhere: sha256 of the compiled reference's result per case, mode and map."""
    rec = recorded()
    assert sorted(rec) == sorted(REACHABLE + MEAN_REF)
    checked = 0
    for name, per_mode in rec.items():
        case = BY_NAME[name]
        got = [digest(g) for g in oracle_results(oracle, case)]
        assert sorted(per_mode) == sorted(str(m) for m in (modes(case) or ["mean"]))
        for mode, want in per_mode.items():
            if case["stage"] == "gap" and mode == str(MIDDLEBURY):
                continue          # (the recorded maps are median-filtered: the reference's filter is not restated)
            assert got == want, f"{name} mode {mode}"
            checked += 1
    assert checked > 40


@needs_ref
def test_the_recorded_digests_are_the_compiled_references():
    rec = recorded()
    for name in REACHABLE:
        for mode in modes(BY_NAME[name]):
            assert rec[name][str(mode)] == [digest(w) for w in reference_results(BY_NAME[name], mode)], (name, mode)
    for name in MEAN_REF:
        assert rec[name]["mean"] == [digest(reference_mean(BY_NAME[name]))], name


# ------------------------------------------------------------------ sizes the reference pipeline cannot be asked about
@pytest.mark.parametrize("name", SMALL + MEAN_SMALL)
def test_small_cases_hold_the_oracles_invariants(oracle, name):
    """Cases on images below 97 x 60 (or with parameters outside the reference's two sets): the oracle, pinned on the larger
    cases above, must at least be consistent with itself here."""
    case = BY_NAME[name]
    got = oracle_results(oracle, case)
    if case["stage"] == "mean":
        assert case["untouched"] and bit_equal(got[0], case["D"])       # fewer rows than the window: the filter writes nothing
        return
    for g, m in zip(got, two_maps(case)):
        if case["stage"] == "seg":          # idempotent; what stays is untouched; the speckle rule on whole components
            again = g.copy()
            oracle.elas_remove_small_segments(again, case["subsampling"], case["speckle_size"], elas_synth.SIM)
            assert bit_equal(again, g)
            assert bit_equal(g, elas_synth.component_model(m, elas_synth.speckle_of(case["speckle_size"], case["subsampling"])))
        elif case["stage"] == "gap":        # valid pixels stay, nothing becomes invalid, a filled pixel lies between the line's values
            valid = m >= 0
            assert bit_equal(g[valid], m[valid])
            if valid.any():
                assert g[g >= 0].max() <= m[valid].max() and g[g >= 0].min() >= m[valid].min()
        else:                               # lr: a pixel keeps its value or goes to -10
            assert ((g == m) | (g == elas_synth.INVALID)).all() and ((g >= 0) <= (m >= 0)).all()


@pytest.mark.parametrize("name", [c["name"] for c in MAP_CASES if c["stage"] == "seg"])
def test_segment_cases_equal_the_component_model(oracle, name):
    """Inside the precondition (every invalid pixel at -10, threshold below 10) the reference's ordered flood fill and the
    connected components of the similarity relation — what the device's union-find computes — are the same partition."""
    case = BY_NAME[name]
    assert ((case["D"] >= 0) | (case["D"] == elas_synth.INVALID)).all()
    got = oracle_results(oracle, case)[0]
    assert bit_equal(got, elas_synth.component_model(case["D"], elas_synth.speckle_of(case["speckle_size"], case["subsampling"])))


def test_maps_with_minus_one_are_outside_remove_small_segments_precondition(oracle):
    """plvs_hip_elas_remove_small_segments documents: every invalid pixel at -10.  Recorded as a fact: with -10 the component
    model equals the oracle on random maps; with a tenth of the pixels at -1 (computeDisparity's 'no match') or at -0.5 it does
    not — in the reference a -1 seed absorbs a neighbouring valid segment of disparity <= threshold - 1 (|-1 - 0| <= 1)."""
    differ = {-10.0: 0, -1.0: 0, -0.5: 0}
    for seed in range(6):
        rng = np.random.default_rng(seed)
        base = rng.choice(np.array([0.0, 1.0, 2.5, 3.5], np.float32), size=(60, 97))
        holes = rng.random(base.shape) < 0.1
        for marker in differ:
            D = base.copy()
            D[rng.random(base.shape) < 0.1] = elas_synth.INVALID
            D[holes] = marker
            got = D.copy()
            oracle.elas_remove_small_segments(got, False, 12, 1.0)
            differ[marker] += int((got != elas_synth.component_model(D, 12)).sum())
    assert differ[-10.0] == 0 and differ[-1.0] > 50 and differ[-0.5] > 50, differ


# ------------------------------------------------------------------ the triangle cases depend on the order of the list
def test_triangle_cases_depend_on_the_order_where_they_should(oracle):
    calls, _ = golden_capture()
    cases = {c["name"]: c for c in elas_synth.triangle_cases(calls)}
    for c in cases.values():
        elas_synth.assert_facts(c)
        for a in c["calls"]:
            sup = a["support"]
            assert (sup["v"] >= 0).all() and (sup["v"] < a["height"]).all()        # (the reference would write outside D)
            assert max(a["tri"][k].max() for k in ("c1", "c2", "c3")) < len(sup)

    def maps(name, **setting):
        return [oracle.elas_compute_disparity(dict(a, subsampling=setting.get("subsampling", 0)),
                                              match_texture=setting.get("match_texture", 1)) for a in cases[name]["calls"]]
    base = maps("tri_capture")
    for b, a in zip(base, calls):
        assert bit_equal(b, a["D"].reshape(b.shape))                                # the capture's own list: the reference's map
    # a Delaunay list shares only edges: its order decides nothing
    assert all(bit_equal(s, b) for s, b in zip(maps("tri_capture_shuffled"), base))
    # overlapping triangles: the last one over a pixel wins, so two orders of the same list give two maps
    for setting in elas_synth.TRI_SETTINGS:
        if setting["match_texture"] == 10000:
            assert all((m == elas_synth.INVALID).all() for m in maps("tri_appended", **setting))    # no pixel has that texture
            continue
        fwd, rev, pre = maps("tri_appended", **setting), maps("tri_appended_reversed", **setting), maps("tri_prepended", **setting)
        scale = 4 if setting["subsampling"] else 1
        for k in range(2):
            assert int((fwd[k] != rev[k]).sum()) > 500 // scale, (setting, k, int((fwd[k] != rev[k]).sum()))
            assert int((fwd[k] != pre[k]).sum()) > 500 // scale
    assert any((m >= 0).any() for m in maps("tri_degenerate_only"))
