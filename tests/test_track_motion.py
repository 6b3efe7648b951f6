"""The motion-model link of the tracking path: the search of Tracking::TrackWithMotionModel (reference src/Tracking.cc:3615-3664) in
one call, with the projection of the last frame's map points and lines (src/ORBmatcher.cc:1805-1820, include/LineProjection.h:144-264)
on the device.  Pinned by the reference's OWN definitions compiled and run on tests/track_motion_scenario.py, recorded in
tests/golden/track_motion_reference.npz by scripts/make_track_motion_golden.py; at other sizes by the numpy restatement that file pins
and by the oracle's search restatement fed those fields.  There is no logarithm on this path and no "ambiguous" class: every float and
every index is compared for equality of bits."""
import ctypes
import json
import os
import re
import struct
import subprocess

import numpy as np
import pytest

from tests import track_motion_restatement as R
from tests import track_motion_scenario as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
ENTRY = "plvs_hip_frame_search_last_frame"
POINT_KEYS = ("proj_valid", "u", "v", "invz")
LINE_KEYS = ("proj_valid", "proj6")
POINT_REACHED = ("invalid", "behind", "z_plus_zero_nan", "z_plus_zero_inf", "nan_accepted", "out_left", "out_right", "out_top", "out_bottom",
                 "on_left", "on_right", "on_top", "on_bottom", "accepted")
LINE_REACHED = ("invalid", "middle_behind", "middle_out_left", "middle_out_right", "middle_out_top", "middle_out_bottom", "too_near", "too_far",
                "on_near_edge", "on_far_edge", "start_behind", "end_behind", "start_out", "end_out", "accepted")


def same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def _facts():
    with open(os.path.join(GOLDEN, "track_motion_reference_facts.json")) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def scenario():
    inp = S.inputs()
    g = np.load(os.path.join(GOLDEN, "track_motion_reference.npz"))
    assert S.inputs_digest(inp) == str(g["inputs_digest"]), "the synthetic inputs changed: regenerate with scripts/make_track_motion_golden.py"
    return inp, {k: g[k] for k in g.files}


@pytest.fixture(scope="module")
def crowd(scenario):
    c = S.crowd_inputs()
    assert S.inputs_digest(c) == str(scenario[1]["crowd_inputs_digest"])
    return c


@pytest.fixture(scope="module")
def minus_zero(scenario):
    m = S.minus_zero_inputs()
    assert S.inputs_digest(m) == str(scenario[1]["minus_zero_inputs_digest"])
    return m


# ---------------------------------------------------------------------------------------------------------------- CPU
def test_inputs_digest_matches(scenario, crowd, minus_zero):
    inp, g = scenario
    d = _facts()["digests"]
    assert d["inputs"] == S.inputs_digest(inp) == str(g["inputs_digest"])
    assert d["crowd_inputs"] == S.inputs_digest(crowd)
    assert d["minus_zero_inputs"] == S.inputs_digest(minus_zero)
    for kind in S.POLICY_KINDS:
        assert d[f"policy_{kind}_inputs"] == S.inputs_digest(S.policy_inputs(kind)) == str(g[f"policy_{kind}_inputs_digest"])
    assert 90 <= len(inp["points"]["valid"]) <= 110 and 24 <= len(inp["lines"]["valid"]) <= 40
    assert len(inp["frame"]["x"]) == 200 and len(inp["frame"]["keylines"]) == 40
    assert abs(float(inp["poses"]["q_cw"][3])) < 0.999      # not the identity


def test_restatement_equals_the_reference(scenario, crowd, minus_zero):
    inp, g = scenario
    cp, cl = {}, {}
    out = R.project_points(inp["poses"], inp["points"], cp)
    for k in ("pc",) + POINT_KEYS:
        assert same(out[k], g["p_" + k]), k
    out = R.project_lines(inp["poses"], inp["lines"], cl)
    for k in LINE_KEYS:
        assert same(out[k], g["l_" + k]), k
    facts = _facts()["facts"]
    assert cp == facts["points"] and cl == facts["lines"]
    outc = R.project_points(crowd["poses"], crowd["points"])
    for k in ("pc",) + POINT_KEYS:
        assert same(outc[k], g["crowd_p_" + k]), k
    cm = {}
    outm = R.project_points(minus_zero["poses"], minus_zero["points"], cm)
    for k in ("pc",) + POINT_KEYS:
        assert same(outm[k], g["minus_zero_p_" + k]), k
    assert cm == facts["points_minus_zero"]
    for d in S.DIRECTIONS:
        for mono in (0, 1):
            assert list(R.direction(S.poses(d, mono))) == facts["directions"][f"{d}_mono{mono}"]


def test_the_golden_run_takes_every_branch(scenario, minus_zero):
    inp, g = scenario
    facts = _facts()["facts"]
    for k in POINT_REACHED:
        assert facts["points"][k] >= 1, k
    for k in LINE_REACHED:
        assert facts["lines"][k] >= 1, k
    # z == -0.0f, in the set of its own: the reference's x3Dc(2) is a zero with the sign bit set, invzc = -inf rejects the point
    # before it is projected; the same point with z == +0.0f goes on to the bounds
    assert facts["points_minus_zero"]["z_minus_zero"] >= 1
    i, j = minus_zero["where"]["z_minus_zero"][0], minus_zero["where"]["z_plus_zero"][0]
    assert g["minus_zero_p_pc"][i, 2].tobytes() == np.float32(-0.0).tobytes() and np.isneginf(g["minus_zero_p_invz"][i])
    assert g["minus_zero_p_proj_valid"][i] == 0 and g["minus_zero_p_u"][i] == -1 and g["minus_zero_p_v"][i] == -1
    assert g["minus_zero_p_pc"][j, 2].tobytes() == np.float32(0.0).tobytes() and np.isposinf(g["minus_zero_p_invz"][j])
    assert g["minus_zero_p_proj_valid"][j] == 0 and np.isneginf(g["minus_zero_p_u"][j])
    assert all(g["minus_zero_p_proj_valid"][k] == 1 for k in minus_zero["where"]["match"])
    assert facts["directions"] == dict(neither_mono0=[0, 0], neither_mono1=[0, 0], forward_mono0=[1, 0], forward_mono1=[0, 0],
                                       backward_mono0=[0, 1], backward_mono1=[0, 0])
    # the point the quaternion action and R p + t disagree on, among the accepted ones: the golden holds the quaternion's bits
    differ = facts["points_where_quaternion_and_matrix_differ"]
    assert len(differ) >= 1
    P = inp["poses"]
    mat = R.project_points(P, inp["points"], act=lambda p: R.matrix_act(P["Rcw"], P["tcw"], p))
    i = differ[0]
    assert g["p_proj_valid"][i] == 1 and (g["p_u"][i].tobytes() != mat["u"][i].tobytes() or g["p_v"][i].tobytes() != mat["v"][i].tobytes())
    w = inp["where"]
    i = w["z_plus_zero_nan"][0]
    assert g["p_proj_valid"][i] == 1 and np.isnan(g["p_u"][i]) and np.isposinf(g["p_invz"][i])
    for k, col, b in (("on_left", "u", 0), ("on_right", "u", 1), ("on_top", "v", 2), ("on_bottom", "v", 3)):
        assert all(g["p_proj_valid"][j] == 1 and g["p_" + col][j] == S.BOUNDS4[b] for j in w[k]), k
    assert all(g["l_proj_valid"][j] == 1 for j in w["line_on_near_edge"] + w["line_on_far_edge"])
    assert all(g["l_proj_valid"][j] == 0 for j in w["line_past_near_edge"] + w["line_past_far_edge"])
    j = w["line_end_out"][0]
    assert g["l_proj_valid"][j] == 0 and (g["l_proj6"][j, :4] != -1).all()      # rejected late: it has gone through every store
    # th, the direction, the orientation check and the occupied flags bite in the searches
    assert len({g[S.search_key(th, 1, 1, d)].tobytes() for th in (7.0, 15.0) for d in S.DIRECTIONS}) == 6
    assert len({g[S.search_key(15.0, c, o, "neither")].tobytes() for c in (0, 1) for o in (0, 1)}) == 4
    assert len({g[S.line_key(1, 1, d)].tobytes() for d in S.DIRECTIONS}) == 3
    pol = facts["policy"]
    assert (pol["plain"]["point_retries"], pol["plain"]["line_retries"]) == (0, 0)
    assert (pol["few_points"]["point_retries"], pol["few_points"]["line_retries"], pol["few_points"]["larger_line_search_used"]) == (1, 0, 1)
    assert (pol["few_lines"]["point_retries"], pol["few_lines"]["line_retries"], pol["few_lines"]["larger_line_search_used"]) == (0, 1, 1)


def test_header_declares_and_library_exports_the_entry(tmp_path):
    with open(os.path.join(ROOT, "include", "plvs_hip.h")) as f:
        header = f.read()
    for name in ("plvs_motion_poses", "plvs_motion_points", "plvs_motion_lines", "plvs_motion_policy", "plvs_motion_result"):
        assert name in header, name
    for cite in ("src/ORBmatcher.cc:1774-1993", "src/LineMatcher.cc:837-1230", "include/LineProjection.h:144-end", "src/Tracking.cc:3615-3664"):
        assert cite in header, cite
    c = tmp_path / "use.c"
    c.write_text('#include "plvs_hip.h"\nint main(void) { plvs_motion_poses m; plvs_motion_points p; plvs_motion_lines l; plvs_motion_policy q;\n'
                 '  plvs_motion_result r; m.n_cameras = 1; p.n = 0; l.n = 0; q.th = 15.0f;\n'
                 '  return plvs_hip_frame_search_last_frame(&m, 0, 0, 0, &p, &l, &q, 0, 0, 0, 0, &r, 0, 0); }\n')
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(c), "-o",
                    str(tmp_path / "use.o")], check=True)
    from plvs_amd import _lib
    lib = _lib.lib
    assert re.search(r"\bint " + ENTRY + r"\(", header), f"{ENTRY} is not declared in include/plvs_hip.h"
    assert hasattr(lib, ENTRY), f"libplvs_hip.so does not export {ENTRY}"
    lib.plvs_hip_abi_version.restype = ctypes.c_int
    assert lib.plvs_hip_abi_version() == 1
    from plvs_amd import frame
    assert callable(frame.search_last_frame)


def _pose_file(path, inp):
    P = inp["poses"]
    pts = inp["points"]
    f32 = lambda a: np.ascontiguousarray(a, np.float32).tobytes()      # noqa: E731
    cases = [S.poses(d, mono) for d in S.DIRECTIONS for mono in (0, 1)]
    with open(path, "wb") as f:
        f.write(struct.pack("<i", len(pts["valid"])) + f32(P["q_cw"]) + f32(P["tcw"]) + f32(pts["pos"]))
        f.write(struct.pack("<i", len(cases)))
        for c in cases:
            f.write(f32(c["q_lw"]) + f32(c["tlw"]) + f32(c["Ow"]) + f32([c["mb"]]) + struct.pack("<i", int(c["mono"])))
    return [f"{d}_mono{mono}" for d in S.DIRECTIONS for mono in (0, 1)]


def _check_pose_program(exe, scenario, tmp_path, env=None, minus_zero=None):
    inp, g = scenario
    if minus_zero is not None:      # the set with z == -0.0f: the sign of the zero is in the bits compared
        names = _pose_file(str(tmp_path / "pose_mz.bin"), minus_zero)
        r = subprocess.run([exe, str(tmp_path / "pose_mz.bin")], capture_output=True, text=True, env=env)
        assert r.returncode == 0 and "track_pose ok" in r.stdout, r.stdout + r.stderr
        pc = np.array([[int(x, 16) for x in l.split()[1:]] for l in r.stdout.splitlines() if l.startswith("pc ")], np.uint32).view(np.float32)
        valid = minus_zero["points"]["valid"] != 0
        assert pc.shape == g["minus_zero_p_pc"].shape and same(pc[valid], g["minus_zero_p_pc"][valid])
        assert pc[minus_zero["where"]["z_minus_zero"][0], 2].tobytes() == np.float32(-0.0).tobytes()
    names = _pose_file(str(tmp_path / "pose.bin"), inp)
    r = subprocess.run([exe, str(tmp_path / "pose.bin")], capture_output=True, text=True, env=env)
    assert r.returncode == 0 and "track_pose ok" in r.stdout, r.stdout + r.stderr
    pc = np.array([[int(x, 16) for x in l.split()[1:]] for l in r.stdout.splitlines() if l.startswith("pc ")], np.uint32).view(np.float32)
    valid = inp["points"]["valid"] != 0
    assert pc.shape == g["p_pc"].shape and same(pc[valid], g["p_pc"][valid]) and valid.sum() > 80      # (the golden holds 0 where not valid)
    dirs = [[int(x) for x in l.split()[1:]] for l in r.stdout.splitlines() if l.startswith("direction ")]
    facts = _facts()["facts"]
    assert dirs == [facts["directions"][k] for k in names] and len(dirs) == 6
    return r


@pytest.mark.parametrize("compiler", ["g++", "/opt/rocm/llvm/bin/clang++"])
def test_pose_header_on_the_host_reproduces_the_reference(scenario, minus_zero, tmp_path, compiler):
    """plvs_amd/csrc/track_pose.hpp — the text the projection kernel compiles — as a stand-alone host program under g++ and under
    ROCm's clang: the golden x3Dc of every valid point, and bForward / bBackward of the three last-frame poses with bMono off and on."""
    if not os.path.exists(compiler) and compiler != "g++":
        pytest.fail(f"{compiler} is missing")
    exe = str(tmp_path / "track_pose_host")
    subprocess.run([compiler, "-std=c++14", "-O2", "-ffp-contract=off", "-Wall", "-Wextra", "-Werror",
                    os.path.join(ROOT, "tests", "host", "track_pose_host.cpp"), "-o", exe], check=True)
    _check_pose_program(exe, scenario, tmp_path, minus_zero=minus_zero)


def test_pose_header_under_host_sanitizers(scenario, tmp_path):
    exe = str(tmp_path / "track_pose_host_san")
    subprocess.run(["g++", "-std=c++14", "-O1", "-g", "-ffp-contract=off", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", os.path.join(ROOT, "tests", "host", "track_pose_host.cpp"), "-o", exe], check=True)
    r = _check_pose_program(exe, scenario, tmp_path, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1"))
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr


# ---------------------------------------------------------------------------------------------------------------- GPU
def _one_call(inp, th=15.0, check=1, occ=1, direction=None, mono=None, lines=True, min_points=0, min_lines=0, has_obs=True):
    from plvs_amd import frame
    poses = inp["poses"] if direction is None else S.poses(direction, 0 if mono is None else mono)
    P, L = dict(inp["points"]), (dict(inp["lines"]) if lines and inp["lines"] is not None else None)
    if not has_obs:
        P["has_obs"] = None
        if L is not None:
            L["has_obs"] = None
    return frame.search_last_frame(poses, S.frame_view(inp), inp["frame"]["cur_angle"], S.line_view(inp) if L is not None else None, P, L, th=th,
                                   nn_ratio_lines=S.NN_RATIO_LINES, check_orientation=bool(check), min_point_matches=min_points,
                                   min_line_matches=min_lines, occupied_points=inp["frame"]["occupied_points"] if occ else None,
                                   occupied_lines=inp["frame"]["occupied_lines"] if occ and L is not None else None)


def _check_fields(got, want_p=None, want_l=None):
    if want_p is not None:
        for k, name in zip(POINT_KEYS, ("proj_valid_points", "u", "v", "invz")):
            assert same(got[name], want_p[k]), k
    if want_l is not None:
        assert same(got["proj_valid_lines"], want_l["proj_valid"]) and same(got["proj6"], want_l["proj6"])


def _golden_fields(g, prefix=""):
    return {k: g[prefix + "p_" + k] for k in POINT_KEYS}, ({k: g["l_" + k] for k in LINE_KEYS} if not prefix else None)


def _existing_points(inp, fields, th, fw, bw, check, occ, has_obs=True):
    from plvs_amd.orbmatcher import LastFrameView, ORBmatcher
    pts = inp["points"]
    lf = LastFrameView(valid=fields["proj_valid"], u=fields["u"], v=fields["v"], invz=fields["invz"], octave=pts["octave"], angle=pts["angle"],
                       desc=pts["desc"], has_obs=pts["has_obs"] if has_obs else None)
    return ORBmatcher(0.9, bool(check)).SearchByProjectionLastFrame(S.frame_view(inp), inp["frame"]["cur_angle"], float(S.BOUNDS4[1]),
                                                                   float(S.BOUNDS4[3]), float(S.MBF), lf, th, bool(fw), bool(bw),
                                                                   occupied=inp["frame"]["occupied_points"] if occ else None)


def _existing_lines(inp, fields, larger, direction, check, occ, has_obs=True):
    from plvs_amd import _lib
    ln = inp["lines"]
    F, keep = S.line_view(inp)
    a = np.full(max(F.n, 1), -7, np.int32)
    n = ctypes.c_int()
    p = lambda x: None if x is None else _lib.np_ptr(np.ascontiguousarray(x))      # noqa: E731
    hold = [np.ascontiguousarray(x) for x in (fields["proj_valid"], fields["proj6"], ln["octave"], ln["angle"], ln["desc"], ln["has_obs"])]
    f = _lib.lib.plvs_hip_lines_search_by_projection_ff
    f.argtypes = [ctypes.c_void_p] * 2 + [ctypes.c_int] + [ctypes.c_void_p] * 6 + [ctypes.c_int, ctypes.c_int, ctypes.c_float, ctypes.c_int] + [ctypes.c_void_p] * 2
    _lib.check(f(ctypes.byref(F), p(inp["frame"]["occupied_lines"]) if occ else None, len(ln["valid"]), *[_lib.np_ptr(h) for h in hold[:5]],
                 _lib.np_ptr(hold[5]) if has_obs else None, int(larger), int(direction), float(S.NN_RATIO_LINES), int(check), _lib.np_ptr(a), ctypes.byref(n)))
    return n.value, a[:F.n]


@pytest.mark.gpu
def test_projection_fields_equal_the_reference(scenario, crowd):
    inp, g = scenario
    got = _one_call(inp)
    gp, gl = _golden_fields(g)
    _check_fields(got, gp, gl)
    facts = _facts()["facts"]
    i = inp["where"]["z_plus_zero_nan"][0]
    print("NaN bits (device, reference):", [hex(int(got[k][i].view(np.uint32))) for k in ("u", "v")], [hex(b) for b in facts["nan_bits"]])
    i = facts["points_where_quaternion_and_matrix_differ"][0]
    assert got["u"][i].tobytes() == g["p_u"][i].tobytes() and got["v"][i].tobytes() == g["p_v"][i].tobytes()
    assert got["stats"] == dict(window_launches=1, point_retries=0, line_retries=0, candidate_spills=0)
    _check_fields(_one_call(crowd, lines=False), _golden_fields(g, "crowd_")[0])


@pytest.mark.gpu
def test_minus_zero_depth_equals_the_reference(scenario, minus_zero):
    """x3Dc(2) == -0.0f: invzc = 1.0 / -0.0 = -inf < 0, the point is rejected before its projection and reports (-1, -1, -inf)."""
    _, g = scenario
    got = _one_call(minus_zero, occ=0, lines=False)
    _check_fields(got, _golden_fields(g, "minus_zero_")[0])
    i, j = minus_zero["where"]["z_minus_zero"][0], minus_zero["where"]["z_plus_zero"][0]
    print("z == -0: u, v, invz, valid =", got["u"][i], got["v"][i], got["invz"][i], got["proj_valid_points"][i], "  z == +0:", got["u"][j], got["invz"][j])
    assert np.isneginf(got["invz"][i]) and got["proj_valid_points"][i] == 0 and got["u"][i] == -1 and got["v"][i] == -1
    assert np.isposinf(got["invz"][j]) and got["proj_valid_points"][j] == 0
    assert same(got["assigned_points"], g["minus_zero_assigned_points"])
    assert got["nmatches_points"] == _facts()["facts"]["nmatches"]["minus_zero_assigned_points"] >= 6
    assert i not in got["assigned_points"] and j not in got["assigned_points"]


@pytest.mark.gpu
@pytest.mark.parametrize("n_lines", [0, 1])
def test_nothing_to_search_follows_the_retry_rules(n_lines):
    """No last-frame point at all: both point searches of Tracking.cc:3626-3640 return 0, so with the minima set the call reports the
    repetition at 2 * th and the larger line search, whether or not there is a line to search — as it does for last-frame points over
    a frame without key points."""
    inp = S.random_inputs(0, n_lines, seed=11, n_kp=300, n_kl=60)
    # (one line finds fewer than 10 matches whatever it finds; the rules never look at more than the count)
    want = R.track_with_motion_model(lambda th: (0, None), lambda larger: (0, None), 15.0, 20, 10, have_lines=n_lines > 0)
    assert (want["point_retries"], want["line_retries"]) == (1, 0)
    got = _one_call(inp, 15.0, 1, 0, min_points=20, min_lines=10)
    assert got["nmatches_points"] == 0 and got["th_used"] == want["th_used"] == 30.0
    assert got["larger_line_search_used"] == want["larger_line_search_used"] == 1
    assert got["stats"] == dict(window_launches=0, point_retries=1, line_retries=0, candidate_spills=0), got["stats"]
    once = _one_call(inp, 15.0, 1, 0)
    assert once["th_used"] == 15.0 and once["larger_line_search_used"] == 0 and once["stats"]["point_retries"] == 0


@pytest.mark.gpu
@pytest.mark.parametrize("th", [7.0, 15.0])
@pytest.mark.parametrize("check", [1, 0])
@pytest.mark.parametrize("occ", [1, 0])
@pytest.mark.parametrize("direction", S.DIRECTIONS)
def test_search_last_frame_equals_the_reference(scenario, th, check, occ, direction):
    inp, g = scenario
    facts = _facts()["facts"]
    got = _one_call(inp, th, check, occ, direction)
    gp, gl = _golden_fields(g)
    _check_fields(got, gp, gl)
    fw, bw = facts["directions"][f"{direction}_mono0"]
    assert (got["forward"], got["backward"]) == (fw, bw) and got["th_used"] == th and got["larger_line_search_used"] == 0
    kp, kl = S.search_key(th, check, occ, direction), S.line_key(check, occ, direction)
    assert same(got["assigned_points"], g[kp]) and got["nmatches_points"] == facts["nmatches"][kp]
    assert same(got["assigned_lines"], g[kl]) and got["nmatches_lines"] == facts["nmatches"][kl]
    assert got["stats"] == dict(window_launches=1, point_retries=0, line_retries=0, candidate_spills=0)
    # ... and what the two existing entries return when fed the reported fields
    n, a = _existing_points(inp, {k: got[v] for k, v in zip(POINT_KEYS, ("proj_valid_points", "u", "v", "invz"))}, th, fw, bw, check, occ)
    assert n == got["nmatches_points"] and same(a, got["assigned_points"])
    n, a = _existing_lines(inp, dict(proj_valid=got["proj_valid_lines"], proj6=got["proj6"]), 0, S.direction_code(fw, bw), check, occ)
    assert n == got["nmatches_lines"] and same(a, got["assigned_lines"])
    # bMono: neither direction, whatever the poses say
    mono = _one_call(inp, th, check, occ, direction, mono=1)
    assert (mono["forward"], mono["backward"]) == (0, 0)
    assert same(mono["assigned_points"], g[S.search_key(th, check, occ, "neither")]) and same(mono["assigned_lines"], g[S.line_key(check, occ, "neither")])


@pytest.mark.gpu
@pytest.mark.parametrize("kind", S.POLICY_KINDS)
def test_retry_rules_equal_the_reference(scenario, kind):
    _, g = scenario
    want = _facts()["facts"]["policy"][kind]
    inp = S.policy_inputs(kind)
    got = _one_call(inp, 15.0, 1, 0, min_points=20, min_lines=10)
    print(kind, got["stats"], want)
    assert same(got["assigned_points"], g[f"policy_{kind}_assigned_points"]) and got["nmatches_points"] == want["nmatches_points"]
    assert same(got["assigned_lines"], g[f"policy_{kind}_assigned_lines"]) and got["nmatches_lines"] == want["nmatches_lines"]
    assert got["th_used"] == want["th_used"] and got["larger_line_search_used"] == want["larger_line_search_used"]
    assert got["stats"] == dict(window_launches=1 + want["point_retries"], point_retries=want["point_retries"], line_retries=want["line_retries"],
                                candidate_spills=0)
    # the minima at 0: one search of each kind, whatever it finds
    once = _one_call(inp, 15.0, 1, 0)
    assert once["stats"]["point_retries"] == 0 == once["stats"]["line_retries"] and once["th_used"] == 15.0 and once["larger_line_search_used"] == 0
    if want["point_retries"]:
        assert once["nmatches_points"] < 20 <= got["nmatches_points"]
    if want["line_retries"]:
        assert once["nmatches_lines"] < 10 <= got["nmatches_lines"]


@pytest.mark.gpu
def test_crowd_takes_the_spill_path(scenario, crowd, oracle):
    _, g = scenario
    m, n = len(crowd["points"]["valid"]), len(crowd["frame"]["x"])
    assert m * n > m * 32 + 4096      # every point's window holds the whole cluster: more candidates than the first capacity
    got = _one_call(crowd, lines=False)
    _check_fields(got, _golden_fields(g, "crowd_")[0])
    assert got["stats"] == dict(window_launches=2, point_retries=0, line_retries=0, candidate_spills=1), got["stats"]
    assert same(got["assigned_points"], g["crowd_assigned_points"]) and got["nmatches_points"] == _facts()["facts"]["nmatches"]["crowd_assigned_points"]
    fields = {k: g["crowd_p_" + k] for k in POINT_KEYS}
    na, a = _existing_points(crowd, fields, 15.0, 0, 0, 1, 1)
    assert na == got["nmatches_points"] and same(a, got["assigned_points"])


@pytest.mark.gpu
@pytest.mark.parametrize("n", [0, 1, 64, 257])
@pytest.mark.parametrize("nl", [0, 1, 65])
def test_sizes_against_the_restatement(oracle, n, nl):
    """257 points cross the workgroup boundary between the two ranges of the grid."""
    inp = S.random_inputs(n, nl, seed=11, n_kp=300, n_kl=60)
    want_p, want_l = R.project_points(inp["poses"], inp["points"]), R.project_lines(inp["poses"], inp["lines"])
    got = _one_call(inp)
    _check_fields(got, want_p, want_l)
    wn, wa = S.oracle_point_search(oracle.lib, inp, want_p, 15.0, 0, 0, 1, 1)
    assert got["nmatches_points"] == wn and same(got["assigned_points"], wa)
    wn, wa = S.oracle_line_search(oracle.lib, inp, want_l, 0, 0, 1, 1)
    assert got["nmatches_lines"] == wn and same(got["assigned_lines"], wa)
    if n >= 64:
        assert got["nmatches_points"] > 20 and 0 < want_p["proj_valid"].sum() < n
    if nl >= 65:
        assert got["nmatches_lines"] > 10 and 0 < want_l["proj_valid"].sum() < nl


@pytest.mark.gpu
@pytest.mark.parametrize("nl", [512, 513])
def test_line_distances_on_both_sides_of_the_matrix_switch(nl):
    """512 last-frame lines over 512 key lines are 2^18 descriptor pairs, the last size at which the candidates' distances are read out
    of the all-pairs matrix launched behind the projection kernel; 513 over 512 take the pair-list launch after the wait.  Either way
    the line search is the stand-alone entry's over the fields the one call reports."""
    n_kl = 512
    assert (nl * n_kl > 2 ** 18) == (nl == 513)
    inp = S.random_inputs(8, nl, seed=11, n_kp=64, n_kl=n_kl)
    got = _one_call(inp)
    _check_fields(got, R.project_points(inp["poses"], inp["points"]), R.project_lines(inp["poses"], inp["lines"]))
    n, a = _existing_lines(inp, dict(proj_valid=got["proj_valid_lines"], proj6=got["proj6"]), 0, S.direction_code(got["forward"], got["backward"]), 1, 1)
    print("line matches:", got["nmatches_lines"], "of", int(got["proj_valid_lines"].sum()), "projected lines")
    assert n == got["nmatches_lines"] and same(a, got["assigned_lines"])
    assert got["nmatches_lines"] > 0


@pytest.mark.gpu
def test_lines_absent(scenario):
    inp, g = scenario
    facts = _facts()["facts"]
    # mbLineTrackerOn off: no last-frame lines, a NULL line view
    got = _one_call(inp, lines=False)
    _check_fields(got, _golden_fields(g)[0])
    assert got["nmatches_lines"] == 0 and len(got["assigned_lines"]) == 0 and len(got["proj6"]) == 0
    k = S.search_key(15.0, 1, 1, "neither")
    assert same(got["assigned_points"], g[k]) and got["nmatches_points"] == facts["nmatches"][k]
    # has_obs NULL: every map element counts as observed
    got = _one_call(inp, has_obs=False)
    n, a = _existing_points(inp, _golden_fields(g)[0], 15.0, 0, 0, 1, 1, has_obs=False)
    assert n == got["nmatches_points"] and same(a, got["assigned_points"])
    n, a = _existing_lines(inp, _golden_fields(g)[1], 0, 0, 1, 1, has_obs=False)
    assert n == got["nmatches_lines"] and same(a, got["assigned_lines"])


@pytest.mark.gpu
def test_bad_requests_are_refused(scenario):
    from plvs_amd import _lib, frame
    inp, _ = scenario
    fv, lv, ang = S.frame_view(inp), S.line_view(inp), inp["frame"]["cur_angle"]
    oct_neg = inp["points"]["octave"].copy()
    oct_neg[inp["where"]["match"][0]] = -1
    loct = inp["lines"]["octave"].copy()
    loct[inp["where"]["line_match"][0]] = S.N_LINE_LEVELS
    cases = [dict(poses=dict(inp["poses"], n_cameras=2)), dict(poses=dict(inp["poses"], camera_model=1)),
             dict(points=dict(inp["points"], octave=oct_neg)), dict(lines=dict(inp["lines"], octave=loct)),
             dict(points=dict(inp["points"], pos=None)), dict(lines=dict(inp["lines"], max_dist=None)), dict(poses=dict(inp["poses"], q_cw=None))]
    for c in cases:
        with pytest.raises(_lib.PlvsHipError) as e:
            frame.search_last_frame(c.get("poses", inp["poses"]), fv, ang, lv, c.get("points", inp["points"]), c.get("lines", inp["lines"]))
        assert e.value.code == _lib.PLVS_ERR_INVALID_ARG and len(str(e.value)) > 10, c.keys()
    with pytest.raises(_lib.PlvsHipError):      # last-frame lines without a line view
        frame.search_last_frame(inp["poses"], fv, ang, None, inp["points"], inp["lines"])
    # an octave that is out of range on a point that is NOT valid is never read
    oct_neg = inp["points"]["octave"].copy()
    oct_neg[inp["where"]["invalid"][0]] = -1
    got = frame.search_last_frame(inp["poses"], fv, ang, lv, dict(inp["points"], octave=oct_neg), inp["lines"], occupied_points=inp["frame"]["occupied_points"],
                                  occupied_lines=inp["frame"]["occupied_lines"], nn_ratio_lines=S.NN_RATIO_LINES)
    assert same(got["assigned_points"], scenario[1][S.search_key(15.0, 1, 1, "neither")])
