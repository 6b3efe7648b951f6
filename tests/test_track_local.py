"""The local-map link of the tracking path: Frame::isInFrustum over the local map points and lines (reference src/Frame.cc:955-1017,
:1033-1142) in one launch, and Tracking::SearchLocalPoints / SearchLocalLines (src/Tracking.cc:4430-4579) in one call.  Pinned by the
reference's OWN run on tests/track_local_scenario.py, recorded in tests/golden/track_local_reference.npz by
scripts/make_track_local_golden.py; at other sizes by the numpy restatement that file pins, and by the two existing search entries fed
those fields.  Every comparison is equality of bits or of integers."""
import ctypes
import json
import os
import re
import subprocess

import numpy as np
import pytest

from tests import track_local_restatement as R
from tests import track_local_scenario as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
ENTRIES = ("plvs_hip_frame_is_in_frustum", "plvs_hip_frame_search_local_map")
POINT_KEYS = ("in_view", "proj_x", "proj_y", "proj_xr", "track_depth", "level", "view_cos")
LINE_KEYS = ("in_view", "proj", "proj_xr", "level", "view_cos")
POINT_REACHED = ("skipped", "behind", "pcz_zero", "out_left", "out_right", "out_top", "out_bottom", "too_near", "too_far", "grazing", "in_view",
                 "level_at_0", "level_above_top", "view_cos_above_998", "view_cos_below_998")
LINE_REACHED = ("skipped", "behind", "out_left", "out_right", "out_top", "out_bottom", "too_near", "near_quirk", "too_far", "grazing", "in_view",
                "end_behind")


def same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def _facts():
    with open(os.path.join(GOLDEN, "track_local_reference_facts.json")) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def scenario():
    inp = S.inputs()
    g = np.load(os.path.join(GOLDEN, "track_local_reference.npz"))
    assert S.inputs_digest(inp) == str(g["inputs_digest"]), "the synthetic inputs changed: regenerate with scripts/make_track_local_golden.py"
    return inp, {k: g[k] for k in g.files}


@pytest.fixture(scope="module")
def crowd(scenario):
    c = S.crowd_inputs()
    assert S.inputs_digest(c) == str(scenario[1]["crowd_inputs_digest"])
    return c


# ---------------------------------------------------------------------------------------------------------------- CPU
def test_inputs_digest_matches(scenario, crowd):
    inp, g = scenario
    facts = _facts()
    assert facts["inputs"] == S.inputs_digest(inp) == str(g["inputs_digest"])
    assert facts["crowd_inputs"] == S.inputs_digest(crowd)
    assert len(inp["points"]["skip"]) == 600 and len(inp["lines"]["skip"]) == 120
    assert len(inp["frame"]["x"]) == 350 and len(inp["frame"]["keylines"]) == 80
    assert np.abs(np.asarray(inp["cam"]["Rcw"]).reshape(3, 3) - np.eye(3)).max() > 0.1      # not the identity


def test_restatement_equals_the_reference(scenario, crowd):
    inp, g = scenario
    counters = {}
    out = R.is_in_frustum(inp["cam"], inp["points"], inp["lines"], counters=counters)
    for k in POINT_KEYS:
        assert same(out["p_" + k], g["p_" + k]), k
    for k in LINE_KEYS:
        assert same(out["l_" + k], g["l_" + k]), k
    facts = _facts()["facts"]
    assert out["n_in_view_points"] == facts["n_in_view_points"] == int(g["p_in_view"].sum())
    assert out["n_in_view_lines"] == facts["n_in_view_lines"] == int(g["l_in_view"].sum())
    assert counters["points"] == facts["points"] and counters["lines"] == facts["lines"]
    outc = R.is_in_frustum(crowd["cam"], crowd["points"], None)
    for k in POINT_KEYS:
        assert same(outc["p_" + k], g["crowd_p_" + k]), k
    assert outc["n_in_view_points"] == facts["crowd_n_in_view_points"] == 200


def test_the_golden_run_takes_every_branch(scenario):
    inp, g = scenario
    facts = _facts()["facts"]
    for k in POINT_REACHED:
        assert facts["points"][k] >= 1, k
    for k in LINE_REACHED:
        assert facts["lines"][k] >= 1, k
    assert facts["points"]["level_below_0"] == 0 == facts["lines"]["level_below_0"]      # unreachable inside the distance band
    assert facts["log_overload"] == "std::log(float)" and facts["double_overload"] is False
    assert facts["points"]["ambiguous"] >= 6 and facts["lines"]["ambiguous"] >= 2
    w = inp["where"]
    assert len(w["ratio_points"]) >= 6 and len(w["ratio_lines"]) >= 2
    assert {int(g["p_level"][i]) - k for i, k, _ in w["ratio_points"]} == {0, 1}      # both sides of the integer
    assert {int(g["l_level"][i]) - k for i, k, _ in w["ratio_lines"] if k == 1} == {0, 1}
    i = w["line_end_behind"][0]
    assert g["l_in_view"][i] == 1 and g["l_proj"][i, 5] < 0
    assert all(g["l_in_view"][i] == 0 for i in w["line_near_quirk"])      # a misreading (0.8f * mfMinDistance) would accept them
    L = inp["lines"]
    mid = (np.float32(0.5) * (L["start"] + L["end"])).astype(np.float32)
    d = R._norm((mid - inp["cam"]["Ow"][None, :]).astype(np.float32))
    assert all(np.float32(0.8) * L["min_dist"][i] <= d[i] < np.float32(0.8) * L["max_dist"][i] for i in w["line_near_quirk"])
    # the far-point cut and the window factor bite in the reference's searches
    assert len({g[S.search_key(th, far, True)].tobytes() for th in (1.0, 3.0, 15.0) for far in (False, True)}) == 6
    assert facts["nmatches"][S.search_key(1.0, False, True)] > 150 and facts["nmatches"][S.line_key(False, True)] > 30


def _build_level_program(tmp_path, name, flags):
    exe = str(tmp_path / name)
    subprocess.run(["g++", "-std=c++14", "-ffp-contract=off", "-Wall", "-Wextra", "-Werror", *flags,
                    os.path.join(ROOT, "tests", "host", "track_level_host.cpp"), "-o", exe], check=True)
    return exe


def test_level_rule_against_both_host_overloads(tmp_path):
    """plvs_amd/csrc/track_level.hpp compiled for the host: 10^6 seeded ratios per factor (1.2, 1.1, 2.0) and the f32 neighbours of
    s^k — where the rule says "unambiguous" its level is the host expression's for both overloads, and it marks < 10^-3."""
    exe = _build_level_program(tmp_path, "track_level_host", ["-O2"])
    r = subprocess.run([exe, "1000000"], capture_output=True, text=True)
    assert r.returncode == 0 and "track_level ok" in r.stdout, r.stdout + r.stderr
    lines = [l for l in r.stdout.splitlines() if l.startswith("factor")]
    assert len(lines) == 3
    for l in lines:
        m = re.search(r"(\d+) ratios, (\d+) marked .* (\d+) of (\d+) neighbours of s\^k marked, (\d+) disagreements", l)
        n, marked, near_marked, near, bad = (int(x) for x in m.groups())
        assert n >= 10 ** 6 and marked / n < 1e-3 and bad == 0 and 0 < near_marked < near, l


def test_level_rule_under_host_sanitizers(tmp_path):
    exe = _build_level_program(tmp_path, "track_level_host_san", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"])
    r = subprocess.run([exe, "200000"], capture_output=True, text=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1"))
    assert r.returncode == 0 and "track_level ok" in r.stdout, r.stdout + r.stderr
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr


def test_restated_rule_equals_the_compiled_one(scenario, tmp_path):
    """tests/track_local_restatement.rule (the source of the golden's ambiguity facts) against plvs::predict_level compiled from
    plvs_amd/csrc/track_level.hpp: level and mark of every ratio the scenario has in view, and of the f32 neighbours of 1.2^k."""
    inp, g = scenario
    out = R.is_in_frustum(inp["cam"], inp["points"], inp["lines"])
    exe = _build_level_program(tmp_path, "track_level_host", ["-O2"])
    near = []
    for k in range(-2, 10):
        r = np.float32(np.exp(k * np.float64(S.LOG_SCALE)))
        near += [S._ulps(r, o) for o in range(-4, 5)]
    hexbits = lambda v: "%08x" % int(np.float32(v).view(np.uint32))      # noqa: E731
    for key, levels, extra in (("p_", S.N_LEVELS, near), ("l_", S.N_LINE_LEVELS, near)):
        ratios = [r for r, v in zip(out[key + "ratio"], out[key + "in_view"]) if v] + extra
        r = subprocess.run([exe, "--marks", hexbits(S.LOG_SCALE), str(levels)] + [hexbits(x) for x in ratios], check=True, capture_output=True, text=True)
        compiled = [tuple(int(x) for x in l.split()) for l in r.stdout.splitlines()]
        assert compiled == [R.rule(x, S.LOG_SCALE, levels) for x in ratios] and len(compiled) == len(ratios) > 100
        assert sum(a for _, a in compiled) >= 4
    assert all(out["p_ambiguous"][i] for i, _, _ in inp["where"]["ratio_points"]) and all(out["l_ambiguous"][i] for i, _, _ in inp["where"]["ratio_lines"])
    assert int(out["p_ambiguous"].sum()) + int(out["l_ambiguous"].sum()) >= 8


def test_header_declares_and_library_exports_the_entries(tmp_path):
    with open(os.path.join(ROOT, "include", "plvs_hip.h")) as f:
        header = f.read()
    for name in ("plvs_track_camera", "plvs_track_points", "plvs_track_lines", "PLVS_CAMERA_PINHOLE"):
        assert name in header, name
    c = tmp_path / "use.c"
    c.write_text('#include "plvs_hip.h"\nint main(void) { plvs_track_camera c; plvs_track_points p; plvs_track_lines l; c.n_cameras = 1; p.m = 0; l.m = 0;\n'
                 '  return plvs_hip_frame_is_in_frustum(&c, &p, &l, 0, 0, 0, 0) + plvs_hip_frame_search_local_map(&c, 0, 0, &p, &l, 1.0f, 0, 0.0f, 0.8f, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0); }\n')
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(c), "-o",
                    str(tmp_path / "use.o")], check=True)
    from plvs_amd import _lib
    lib = _lib.lib
    for name in ENTRIES:
        assert re.search(r"\bint " + name + r"\(", header), f"{name} is not declared in include/plvs_hip.h"
        assert hasattr(lib, name), f"libplvs_hip.so does not export {name}"
    lib.plvs_hip_abi_version.restype = ctypes.c_int
    assert lib.plvs_hip_abi_version() == 1
    from plvs_amd import frame
    assert callable(frame.is_in_frustum) and callable(frame.search_local_map)


# ---------------------------------------------------------------------------------------------------------------- GPU
def _check_fields(got, want, points=True, lines=True):
    if points:
        for k in POINT_KEYS:
            assert same(got["points"][k], want["p_" + k]), k
        assert got["n_in_view_points"] == int(np.asarray(want["p_in_view"]).sum())
    if lines:
        for k in LINE_KEYS:
            assert same(got["lines"][k], want["l_" + k]), k
        assert got["n_in_view_lines"] == int(np.asarray(want["l_in_view"]).sum())


def _existing_points(inp, fields, th, far, occ, has_obs=True):
    from plvs_amd.orbmatcher import ORBmatcher
    M = S.mappoint_view(inp["points"], fields)
    if not has_obs:
        M.has_obs = None
    return ORBmatcher(S.NN_RATIO).SearchByProjection(S.frame_view(inp), M, th, far, float(S.TH_FAR),
                                                     occupied=inp["frame"]["occupied_points"] if occ else None)


def _existing_lines(inp, fields, larger, occ, has_obs=True):
    from plvs_amd.linematcher import LineMatcher
    L = inp["lines"]
    return LineMatcher(S.NN_RATIO).SearchByProjection(S.line_view(inp), fields["l_in_view"], fields["l_proj"], fields["l_level"], L["desc"],
                                                      occupied=inp["frame"]["occupied_lines"] if occ else None,
                                                      has_obs=L["has_obs"] if has_obs else None, bLargerSearch=larger)


def _one_call(inp, th=1.0, far=False, larger=False, occ=True, has_obs=True, lines=True):
    from plvs_amd import frame
    P, L = dict(inp["points"]), (dict(inp["lines"]) if lines and inp["lines"] is not None else None)
    if not has_obs:
        P["has_obs"] = None
        if L is not None:
            L["has_obs"] = None
    return frame.search_local_map(inp["cam"], S.frame_view(inp), S.line_view(inp) if L is not None else None, P, L, th=th, far_points=far,
                                  th_far=float(S.TH_FAR), nn_ratio=S.NN_RATIO, larger_search=larger,
                                  occupied_points=inp["frame"]["occupied_points"] if occ else None,
                                  occupied_lines=inp["frame"]["occupied_lines"] if occ and L is not None else None)


@pytest.mark.gpu
def test_is_in_frustum_equals_the_reference(scenario):
    from plvs_amd import frame
    inp, g = scenario
    got = frame.is_in_frustum(inp["cam"], inp["points"], inp["lines"])
    _check_fields(got, g)
    facts = _facts()["facts"]
    assert got["n_in_view_points"] == facts["n_in_view_points"] and got["n_in_view_lines"] == facts["n_in_view_lines"]
    print("stats:", got["stats"])
    assert got["stats"]["ambiguous_points"] + got["stats"]["ambiguous_lines"] >= 8
    for i, _, _, level in facts["ratio_points"]:
        assert got["points"]["level"][i] == level
    for i, _, _, level in facts["ratio_lines"]:
        assert got["lines"]["level"][i] == level
    # either kind alone
    _check_fields(frame.is_in_frustum(inp["cam"], inp["points"], None), g, lines=False)
    _check_fields(frame.is_in_frustum(inp["cam"], None, inp["lines"]), g, points=False)


@pytest.mark.gpu
@pytest.mark.parametrize("th", [1.0, 3.0, 15.0])
@pytest.mark.parametrize("far", [False, True])
@pytest.mark.parametrize("larger", [False, True])
@pytest.mark.parametrize("occ", [True, False])
def test_search_local_map_equals_the_reference(scenario, th, far, larger, occ):
    inp, g = scenario
    facts = _facts()["facts"]
    got = _one_call(inp, th, far, larger, occ)
    _check_fields(got, g)
    assert same(got["assigned_points"], g[S.search_key(th, far, occ)]) and got["nmatches_points"] == facts["nmatches"][S.search_key(th, far, occ)]
    assert same(got["assigned_lines"], g[S.line_key(larger, occ)]) and got["nmatches_lines"] == facts["nmatches"][S.line_key(larger, occ)]
    # ... and what the two existing entries return when fed the golden fields
    n, a = _existing_points(inp, g, th, far, occ)
    assert n == got["nmatches_points"] and same(a, got["assigned_points"])
    n, a = _existing_lines(inp, g, larger, occ)
    assert n == got["nmatches_lines"] and same(a, got["assigned_lines"])
    # one launch of the windows; one more only for points whose level the host decided otherwise (levels_changed counts lines too,
    # and a changed point beyond the far-point cut is not searched)
    assert 1 <= got["stats"]["window_launches"] <= 1 + (1 if got["stats"]["levels_changed"] else 0)
    # has_obs NULL (every map element counts as observed)
    got = _one_call(inp, th, far, larger, occ, has_obs=False)
    n, a = _existing_points(inp, g, th, far, occ, has_obs=False)
    assert n == got["nmatches_points"] and same(a, got["assigned_points"])
    n, a = _existing_lines(inp, g, larger, occ, has_obs=False)
    assert n == got["nmatches_lines"] and same(a, got["assigned_lines"])


@pytest.mark.gpu
def test_crowd_takes_the_spill_path(scenario, crowd):
    _, g = scenario
    m, n = len(crowd["points"]["skip"]), len(crowd["frame"]["x"])
    assert m * n > m * 32 + 4096      # every point's window holds the whole cluster: more candidates than the first capacity
    got = _one_call(crowd, lines=False)
    for k in POINT_KEYS:
        assert same(got["points"][k], g["crowd_p_" + k]), k
    assert got["stats"]["window_launches"] == 2, got["stats"]
    assert same(got["assigned_points"], g["crowd_assigned_points"]) and got["nmatches_points"] == _facts()["facts"]["nmatches"]["crowd_assigned_points"]
    fields = {"p_" + k: g["crowd_p_" + k] for k in POINT_KEYS}
    na, a = _existing_points(crowd, fields, 1.0, False, True)
    assert na == got["nmatches_points"] and same(a, got["assigned_points"])


@pytest.mark.gpu
@pytest.mark.parametrize("m", [0, 1, 64, 257])
@pytest.mark.parametrize("ml", [0, 1, 65])
def test_sizes_against_the_restatement(scenario, m, ml):
    from plvs_amd import frame
    inp, _ = scenario
    sub = S.prefix(inp, m, ml)
    want = R.is_in_frustum(sub["cam"], sub["points"], sub["lines"])
    got = frame.is_in_frustum(sub["cam"], sub["points"], sub["lines"])
    _check_fields(got, want)
    got = _one_call(sub)
    _check_fields(got, want)
    n, a = _existing_points(sub, want, 1.0, False, True)
    assert n == got["nmatches_points"] and same(a, got["assigned_points"])
    n, a = _existing_lines(sub, want, False, True)
    assert n == got["nmatches_lines"] and same(a, got["assigned_lines"])
    if m >= 64:
        assert got["nmatches_points"] > 20
    if ml >= 65:
        assert got["nmatches_lines"] > 20


@pytest.mark.gpu
@pytest.mark.parametrize("ml", [512, 513])
def test_line_distances_on_both_sides_of_the_matrix_switch(ml):
    """512 map lines over 512 key lines are 2^18 descriptor pairs, the last size at which the candidates' distances are read out of
    the all-pairs matrix launched behind the frustum kernel; 513 over 512 take the pair-list launch after the wait.  Either way the
    line search is the stand-alone entry's over the fields the one call reports."""
    n_kl = 512
    assert (ml * n_kl > 2 ** 18) == (ml == 513)
    inp = S.random_inputs(m=8, ml=ml, seed=7, n_kp=64, n_kl=n_kl)
    want = R.is_in_frustum(inp["cam"], inp["points"], inp["lines"])
    got = _one_call(inp)
    _check_fields(got, want)
    fields = {"l_" + k: got["lines"][k] for k in LINE_KEYS}
    n, a = _existing_lines(inp, fields, False, True)
    print("line matches:", got["nmatches_lines"], "of", int(want["l_in_view"].sum()), "map lines in view")
    assert n == got["nmatches_lines"] and same(a, got["assigned_lines"])
    assert got["nmatches_lines"] > 0


@pytest.mark.gpu
def test_lines_absent_and_closed_gates(scenario):
    inp, g = scenario
    facts = _facts()["facts"]
    # mbLineTrackerOn off: no map lines, a NULL line view
    got = _one_call(inp, lines=False)
    _check_fields(got, g, lines=False)
    assert got["lines"] is None and got["n_in_view_lines"] == 0 and got["nmatches_lines"] == 0 and len(got["assigned_lines"]) == 0
    assert same(got["assigned_points"], g[S.search_key(1.0, False, True)])
    # nToMatch == 0 for the points only: nothing of theirs is searched, the lines are
    closed = dict(inp, points=dict(inp["points"], skip=np.ones(600, np.uint8)))
    got = _one_call(closed)
    assert got["n_in_view_points"] == 0 and got["nmatches_points"] == 0 and (got["assigned_points"] == -1).all()
    assert same(got["assigned_lines"], g[S.line_key(False, True)]) and got["nmatches_lines"] == facts["nmatches"][S.line_key(False, True)]
    # ... and for the lines only
    closed = dict(inp, lines=dict(inp["lines"], skip=np.ones(120, np.uint8)))
    got = _one_call(closed)
    assert got["n_in_view_lines"] == 0 and got["nmatches_lines"] == 0 and (got["assigned_lines"] == -1).all()
    assert same(got["assigned_points"], g[S.search_key(1.0, False, True)])


@pytest.mark.gpu
def test_forced_level_change_reruns_the_window(scenario):
    """A marked point whose device-side choice is turned to the other side of the integer (the test hook): the host's expression
    puts the reference's level back, the windows of that point run again, and the result is the golden's."""
    from plvs_amd import frame
    inp, g = scenario
    facts = _facts()["facts"]
    base = _one_call(inp)["stats"]
    # a marked point the reference matches, on which float and double logarithm agree (so the device's own choice is the reference's)
    matched = set(int(v) for v in g[S.search_key(1.0, False, True)])
    idx = [i for i, _, _, _ in facts["ratio_points"] if i in matched and i not in facts["ratio_points_where_the_two_overloads_differ"]][0]
    frame.track_test_flip(idx)
    try:
        got = _one_call(inp)
    finally:
        frame.track_test_flip(-1)
    _check_fields(got, g)
    print("stats without / with the flip:", base, got["stats"])
    assert got["stats"]["levels_changed"] == base["levels_changed"] + 1 and got["stats"]["window_launches"] == 2
    assert same(got["assigned_points"], g[S.search_key(1.0, False, True)]) and got["nmatches_points"] == facts["nmatches"][S.search_key(1.0, False, True)]
    assert idx in got["assigned_points"]      # the flipped point is matched, at the reference's level


@pytest.mark.gpu
def test_bad_requests_are_refused(scenario):
    from plvs_amd import _lib, frame
    inp, _ = scenario
    cases = [dict(cam=dict(inp["cam"], n_cameras=2)), dict(cam=dict(inp["cam"], camera_model=1)), dict(cam=dict(inp["cam"], n_levels=-3)),
             dict(cam=dict(inp["cam"], n_line_levels=-1)), dict(cam=dict(inp["cam"], n_levels=0))]
    for c in cases:
        with pytest.raises(_lib.PlvsHipError) as e:
            frame.is_in_frustum(c["cam"], inp["points"], inp["lines"])
        assert e.value.code == _lib.PLVS_ERR_INVALID_ARG and len(str(e.value)) > 10
        with pytest.raises(_lib.PlvsHipError) as e:
            frame.search_local_map(c["cam"], S.frame_view(inp), S.line_view(inp), inp["points"], inp["lines"])
        assert e.value.code == _lib.PLVS_ERR_INVALID_ARG
    # NULL arrays with non-zero counts, straight through the ABI; nothing is written
    L, p = _lib.lib, _lib.np_ptr
    cc, keep = frame._track_camera(inp["cam"])
    pc, pk, po = frame._track_points(inp["points"])
    for o in po.values():
        o[:] = 77
    for field in ("pos", "skip", "max_dist", "proj_x", "level"):
        saved = getattr(pc, field)
        setattr(pc, field, None)
        nv = ctypes.c_int(-5)
        assert L.plvs_hip_frame_is_in_frustum(ctypes.byref(cc), ctypes.byref(pc), None, ctypes.byref(nv), None, None, None) == _lib.PLVS_ERR_INVALID_ARG
        assert nv.value == -5 and all((o == 77).all() for o in po.values())
        setattr(pc, field, saved)
    with pytest.raises(_lib.PlvsHipError):      # map lines without a line view
        frame.search_local_map(inp["cam"], S.frame_view(inp), None, inp["points"], inp["lines"])
