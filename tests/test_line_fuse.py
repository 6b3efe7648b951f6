"""The search stage of LineMatcher::Fuse for K key frames x M lines in one call (plvs_hip_line_fuse_search, its host twin
plvs_hip_line_fuse_search_host, plvs_amd/csrc/line_fuse_pair.hpp) against the reference's own compiled definitions
(tests/golden/line_fuse_reference.npz, scripts/make_line_fuse_golden.py), the replay rule of INTEGRATION.md 2j on a toy map
(tests/line_fuse_replay.py), and the one-wait entry for points and lines together (plvs_hip_fuse_search_points_and_lines).  Every
index, distance and stage is compared for equality."""
import ctypes
import dataclasses
import json
import os
import re
import struct
import subprocess

import numpy as np
import pytest

from tests import line_fuse_replay as P
from tests import line_fuse_restatement as R
from tests import line_fuse_scenario as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "line_fuse_reference.npz")
FACTS = os.path.join(ROOT, "tests", "golden", "line_fuse_reference_facts.json")
OUTPUTS = ("best_idx", "best_dist", "reached")
ENTRIES = ("plvs_hip_line_fuse_search", "plvs_hip_line_fuse_search_host", "plvs_hip_fuse_search_points_and_lines")


@pytest.fixture(scope="module")
def golden():
    g = dict(np.load(GOLDEN))
    for pre in ("", "crowd_"):      # the entries' outputs from the recorded bestIdx / bestDist
        cand = g[pre + "reached"] == R.CANDIDATE
        g[pre + "best_idx"] = np.where(cand, g[pre + "raw_best_idx"], -1).astype(np.int32)
        g[pre + "best_dist"] = np.where(cand, g[pre + "raw_best_dist"], -1).astype(np.int32)
    return g


@pytest.fixture(scope="module")
def facts():
    with open(FACTS) as fh:
        return json.load(fh)


@pytest.fixture(scope="module")
def scenario():
    return S.inputs()


@pytest.fixture(scope="module")
def crowd():
    return S.crowd_inputs()


@pytest.fixture(scope="module")
def ambiguous():
    inp = S.ambiguous_inputs()
    c = {}
    return inp, R.fuse_search(inp["kfs"], inp["lines"], inp["skip"], inp["th"], c), c


@pytest.fixture(scope="module")
def restated(scenario, crowd):
    return (R.fuse_search(scenario["kfs"], scenario["lines"], scenario["skip"], scenario["th"]),
            R.fuse_search(crowd["kfs"], crowd["lines"], None, crowd["th"]))


def _search(inp, host, skip="own", **kw):
    from plvs_amd.linematcher import LineMatcher
    kfs, lines = S.views(inp)
    return LineMatcher().FuseSearch(kfs, lines, inp["th"], inp["skip"] if isinstance(skip, str) else skip, host=host, **kw)


def _same(out, want, keys=OUTPUTS, what=""):
    for k in keys:
        a, b = np.asarray(out[k]), np.asarray(want[k])
        assert a.shape == b.shape and (a == b).all(), f"{what}{k} differs at {np.argwhere(a != b)[:8].tolist()}"


def _window_pairs(r):
    return int((np.asarray(r["reached"]) >= R.EMPTY_WINDOW).sum())


# ---------------------------------------------------------------------------------------------------------------- CPU

def test_scenario_digests_match_the_golden(scenario, crowd, golden, facts):
    assert S.digest(scenario) == str(golden["inputs_digest"]) == facts["digests"]["inputs"]
    assert S.digest(crowd) == str(golden["crowd_inputs_digest"]) == facts["digests"]["crowd_inputs"]


def test_restatement_equals_the_golden(restated, golden):
    for pre, r in zip(("", "crowd_"), restated):
        for k in ("reached", "raw_best_dist", "n_dist", "level", "n_proj", "proj", "best_idx", "best_dist"):
            a, b = r[k], golden[pre + k]
            assert a.dtype == b.dtype and a.tobytes() == b.tobytes(), pre + k
        # bestIdx is observable in the reference where bestDist <= TH_LOW only (GetMapLine(bestIdx))
        assert (golden[pre + "raw_best_idx"] == r["best_idx"]).all()


def test_golden_run_takes_every_stage_and_every_placed_case(scenario, golden, facts):
    F = facts["facts"]
    counts, w = F["counts"], scenario["where"]
    for code, name in enumerate(R.REACHED):
        if name == "degenerate":        # undefined in the reference: its run has none (test_the_two_undefined_cases_get_their_code)
            assert counts[name] == 0 and not (golden["reached"] == code).any()
            continue
        assert counts[name] >= 1 and int((golden["reached"] == code).sum()) == counts[name], name
    for name in ("dropped_below_level", "dropped_above_level", "dropped_start_gate_alone", "dropped_end_gate_alone", "dropped_right_gate_alone",
                 "u_right_start_zero_stereo_branch", "u_right_end_negative_skips_stereo", "u_right_empty", "split_at_minus_half_pi",
                 "split_at_plus_half_pi", "split_members_on_both_sides", "clipped_column_0", "clipped_column_159", "window_misses_grid",
                 "tie_winner_in_wrapped_part_higher_index", "best_dist_60", "best_dist_61"):
        assert counts[name] >= 1, name
    assert F["crowd_counts"]["beyond_member_64"] >= 1 and F["crowd_counts"]["candidate"] == 8
    assert F["log_overload"] == "std::log(float)" and F["log_double_overload"] == 0
    assert F["atan2_overload"] == "atan2f" and F["atan2_double_overload"] == 0
    assert F["defines"]["USE_ENDPOINTS_AVERAGING"] == 0 and F["defines"]["TH_LOW"] == 60       # the replay rule rests on the first
    at = lambda name, k=0, j=0: int(golden["reached"][k, w[name][j]])
    kf0 = scenario["kfs"][0]
    # key frame 0 holds the placed key lines only: which gate dropped the one in-band member of a slot is the case's own
    for n in ("above_level", "below_level", "start_gate", "end_gate", "right_gate", "u_right_start_zero"):
        assert at(n) == R.NO_CANDIDATE and int(golden["n_dist"][0, w[n][0]]) == 0, n
    for n in ("candidate_mono", "u_right_end_negative", "dist_60", "clip_column_0", "clip_column_159", "split_minus", "split_plus_tie"):
        assert at(n) == R.CANDIDATE, n
    assert at("dist_61") == R.ABOVE_TH_LOW and int(golden["raw_best_dist"][0, w["dist_61"][0]]) == 61
    assert int(golden["best_dist"][0, w["dist_60"][0]]) == 60
    assert at("empty_window") == R.EMPTY_WINDOW and at("window_misses_grid", 2) == R.EMPTY_WINDOW
    assert (kf0["u_right_start"] == 0).sum() == 1                  # mvuRightLineStart == 0.0f takes the stereo branch: `> 0` would
    j = int(np.flatnonzero(kf0["u_right_start"] == 0)[0])          # have skipped it, and the line coincides with the projection
    assert kf0["u_right_end"][j] >= 0
    j = int(golden["best_idx"][0, w["u_right_end_negative"][0]])   # a start that would fail the right-image gate, skipped
    assert kf0["u_right_start"][j] >= 0 and kf0["u_right_end"][j] < 0
    assert scenario["kfs"][1]["u_right_start"] is None             # an empty mvuRightLineStart
    ja, jb = w["tie_indices"]
    assert ja > jb and int(golden["raw_best_idx"][0, w["split_plus_tie"][0]]) == ja and int(golden["n_dist"][0, w["split_plus_tie"][0]]) == 2
    assert int(golden["raw_best_idx"][0, w["split_minus"][0]]) == w["split_minus_members"][0]
    for members in (w["tie_indices"], w["split_minus_members"]):   # on both sides of the wrap, d of opposite signs
        reps = [R.representation(*[kf0["kl"][c][m] for c in ("startPointX", "startPointY", "endPointX", "endPointY")]) for m in members]
        assert reps[0][2] * reps[1][2] < 0 and reps[0][1] * reps[1][1] < 0
    grid2 = R.grid_of(scenario["kfs"][2])
    assert len(grid2[1]) < len(scenario["kfs"][2]["kl"])           # key lines that PosLineInGrid leaves out of the grid
    for n in ("middle_behind", "middle_outside", "too_near", "too_far", "end_behind", "view_angle"):
        assert at(n) == getattr(R, n.upper()), n
    assert [at("end_outside", 0, j) for j in (0, 1)] == [R.END_OUTSIDE] * 2
    assert [int(golden["n_proj"][0, i]) for i in w["end_outside"]] == [3, 2]      # the end's projection outside; the start's


def test_host_entry_equals_the_golden(scenario, crowd, golden):
    out = _search(scenario, host=True)
    _same(out, golden)
    assert out["stats"].tolist() == [0, _window_pairs(golden), 0]
    _same(_search(crowd, host=True), {k: golden["crowd_" + k] for k in OUTPUTS}, what="crowd ")


@pytest.mark.parametrize("shape", [(3, 300, 300, None), (2, 65, 100, 1), (1, 1, 1, None), (3, 63, 0, None)])
def test_host_entry_equals_the_restatement_at_other_sizes(shape):
    K, M, N, empty = shape
    inp = S.random_inputs(K, M, N, seed=K + M, empty_kf=empty)
    _same(_search(inp, host=True), R.fuse_search(inp["kfs"], inp["lines"], inp["skip"], inp["th"]))


def test_host_entry_takes_the_ambiguous_pairs_through_the_hosts_functions(ambiguous):
    """Levels whose quotient lies at an integer and thetas whose window edge lies at a row edge: the restatement calls the C
    library's logf and atan2f, as the compiled reference does (the generator held it against the reference on this very set)."""
    inp, want, c = ambiguous
    assert c["ambiguous_level"] >= 1 and c["ambiguous_theta"] >= 12
    assert want["ambiguous"][0, inp["where"]["ambiguous_theta"]].all()
    _same(_search(inp, host=True), want)


def test_the_two_undefined_cases_get_their_code():
    """distMiddlePoint == 0 (the ratio of PredictScale is 0 / 0) and projected end points that coincide in f32 (the normal is 0 * inf,
    theta a NaN, the cell index an int cast of it) are undefined in the reference; the entries report PLVS_LINE_FUSE_DEGENERATE."""
    inp = S.degenerate_inputs()
    c = {}
    want = R.fuse_search(inp["kfs"], inp["lines"], None, inp["th"], c)
    assert c["dist_zero"] == 1 and c["end_points_coincide"] == 1
    assert want["reached"][0, :2].tolist() == [R.DEGENERATE, R.DEGENERATE]
    out = _search(inp, host=True)
    _same(out, want)
    assert (out["best_idx"][0, :2] == -1).all()


def _wide_theta(scenario):
    """Key frame 1 with a scale factor of 10 at level 1: deltaTheta = 100 degrees, wider than the reference's search allows."""
    kfs = [dict(kf) for kf in scenario["kfs"]]
    kfs[1]["scale_factors"] = np.array([1.0, 10.0, 1.44], np.float32)
    return dict(scenario, kfs=kfs)


def _refusals(scenario, host):
    from plvs_amd import _lib
    from plvs_amd.linematcher import LineMatcher
    kfs, lines = S.views(scenario)
    for change in (dict(n_cameras=2), dict(camera_model=1)):
        bad = [kfs[0], dataclasses.replace(kfs[1], **change), kfs[2]]
        with pytest.raises(_lib.PlvsHipError) as e:
            LineMatcher().FuseSearch(bad, lines, 3.0, scenario["skip"], host=host)
        assert e.value.code == _lib.PLVS_ERR_INVALID_ARG
    with pytest.raises(_lib.PlvsHipError) as e:
        LineMatcher().FuseSearch(kfs, lines, 3.0, scenario["skip"], host=host, outputs=False)
    assert e.value.code == _lib.PLVS_ERR_INVALID_ARG
    with pytest.raises(_lib.PlvsHipError) as e:
        LineMatcher().FuseSearch(kfs, lines, -1.0, scenario["skip"], host=host)
    assert e.value.code == _lib.PLVS_ERR_INVALID_ARG


def test_host_entry_refuses_what_the_device_entry_refuses(scenario):
    from plvs_amd import _lib
    _refusals(scenario, host=True)
    wide = _wide_theta(scenario)
    assert (R.fuse_search(wide["kfs"], wide["lines"], wide["skip"], wide["th"])["reached"] == R.FULL_THETA).any()
    with pytest.raises(_lib.PlvsHipError) as e:
        _search(wide, host=True)
    assert e.value.code == _lib.PLVS_ERR_INVALID_ARG and "theta" in str(e.value)


def _write_pair_input(path, inp):
    K, M = len(inp["kfs"]), len(inp["lines"]["max_dist"])
    f32 = lambda a: np.ascontiguousarray(a, np.float32).tobytes()
    with open(path, "wb") as f:
        f.write(struct.pack("<iif", K, M, inp["th"]))
        for kf in inp["kfs"]:
            kl = kf["kl"]
            f.write(f32(kf["Rcw"]) + f32(kf["tcw"]) + f32(kf["Ow"]) + f32(kf["K4"]) + f32([kf["mbf"]]) + f32(kf["bounds4"]) +
                    f32([kf["max_diag"], kf["log_scale_factor"]]))
            has_right = kf["u_right_start"] is not None
            f.write(struct.pack("<iii", len(kf["scale_factors"]), len(kl), int(has_right)))
            f.write(f32(np.stack([kl["startPointX"], kl["startPointY"], kl["endPointX"], kl["endPointY"]], 1)))
            f.write(np.ascontiguousarray(kl["octave"], np.int32).tobytes())
            if has_right:
                f.write(f32(kf["u_right_start"]) + f32(kf["u_right_end"]))
            f.write(np.ascontiguousarray(kf["desc"], np.uint8).tobytes() + f32(kf["scale_factors"]) + f32(kf["inv_level_sigma2"]))
        p = inp["lines"]
        f.write(b"".join(f32(p[k]) for k in ("start", "end", "normal", "max_dist")))
        f.write(np.ascontiguousarray(p["desc"], np.uint8).tobytes())
        f.write(np.ascontiguousarray(inp["skip"] if inp["skip"] is not None else np.zeros((K, M)), np.uint8).tobytes())


def _run_pair_program(exe, inp, want, tmp_path, env=None):
    path = str(tmp_path / "line_fuse_pair_input.bin")
    _write_pair_input(path, inp)
    r = subprocess.run([exe, path], capture_output=True, text=True, env=env)
    assert r.returncode == 0 and "line_fuse_pair ok" in r.stdout, r.stderr + r.stdout[-500:]
    got = np.array([[int(c) for c in ln.split()[1:]] for ln in r.stdout.splitlines() if ln.startswith("pair ")], np.int64)
    exp = np.stack([np.asarray(want[k]).reshape(-1).astype(np.int64) for k in OUTPUTS], 1)
    assert got.shape == exp.shape and (got == exp).all(), np.argwhere(got != exp)[:8]
    marked, windows = (int(x) for x in re.search(r"marked (\d+) of (\d+)", r.stdout).groups())
    return r, marked, windows


FLAGS = ["-std=c++14", "-ffp-contract=off", "-Wall", "-Wextra", "-Werror"]
HOST_SRC = os.path.join(ROOT, "tests", "host", "line_fuse_pair_host.cpp")


@pytest.mark.parametrize("compiler", ["g++", "/opt/rocm/llvm/bin/clang++"])
def test_pair_header_on_the_host_reproduces_the_reference(scenario, ambiguous, golden, tmp_path, compiler):
    """plvs_amd/csrc/line_fuse_pair.hpp — the text the kernel compiles — as a stand-alone host program under g++ and ROCm's clang:
    the host path equals the golden, and the kernel's rule, walked serially, equals it wherever it does not hand the pair over."""
    if not os.path.exists(compiler) and compiler != "g++":
        pytest.fail(f"{compiler} is missing")
    exe = str(tmp_path / "line_fuse_pair_host")
    subprocess.run([compiler, "-O2"] + FLAGS + [HOST_SRC, "-o", exe], check=True)
    _run_pair_program(exe, scenario, golden, tmp_path)
    inp, want, c = ambiguous
    _, marked, _ = _run_pair_program(exe, inp, want, tmp_path)
    assert marked >= c["ambiguous_theta"]          # (the level's marks on top)


def test_pair_header_under_the_sanitizers(scenario, golden, tmp_path):
    exe = str(tmp_path / "line_fuse_pair_host_san")
    subprocess.run(["g++", "-O1", "-g"] + FLAGS + ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", HOST_SRC, "-o", exe], check=True)
    r, _, _ = _run_pair_program(exe, scenario, golden, tmp_path, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1"))
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr


def _steps(a, b):
    """The number of f32 values from a to b."""
    o = lambda x: (lambda i: np.where(i < 0, np.int64(-2 ** 31) - i, i))(np.asarray(x, np.float32).view(np.int32).astype(np.int64))
    return np.abs(o(a) - o(b))


def test_the_hosts_arctangent_stays_within_the_bound_k_rests_on(tmp_path, capsys):
    """kThetaUlps (line_fuse_pair.hpp) rests on the host's atan2f lying at most ONE f32 step from the correctly rounded value.
    Measured here over a seeded sample of unit normals (nx >= 0, as GetLine2dRepresentation forms them) against atan2l rounded to
    f32; the kernel's own theta — an f64 arctangent rounded to f32 — is held to the same bound with numpy's f64 arctan2 standing
    in.  The marked fraction is counted and printed, on the 839 windows of a random scenario; nothing is asserted about it."""
    rng = np.random.default_rng(S.SEED + 99)
    n = 60000
    ang = np.concatenate([rng.uniform(-np.pi / 2, np.pi / 2, n - 2000), rng.uniform(-1e-3, 1e-3, 1000),
                          np.pi / 2 - np.abs(rng.uniform(0, 1e-3, 500)), -np.pi / 2 + np.abs(rng.uniform(0, 1e-3, 500))])
    nx, ny = np.cos(ang).astype(np.float32), np.sin(ang).astype(np.float32)
    host = np.array([R.atan2_host(y, x) for y, x in zip(ny, nx)], np.float32)
    exact = np.arctan2(ny.astype(np.longdouble), nx.astype(np.longdouble))
    assert np.finfo(np.longdouble).nmant >= 63, "no extended precision to round from"
    cr = exact.astype(np.float32)
    dev_host, dev_f64 = _steps(host, cr), _steps(np.arctan2(ny.astype(np.float64), nx.astype(np.float64)).astype(np.float32), cr)
    assert int(dev_host.max()) <= 1, f"atan2f lies {int(dev_host.max())} f32 steps from the correctly rounded value"
    assert int(dev_f64.max()) <= 1
    assert int(dev_host.max()) + int(dev_f64.max()) <= R.THETA_ULPS // 2            # k = 4: twice the two bounds together
    exe = str(tmp_path / "line_fuse_pair_host")
    subprocess.run(["g++", "-O2"] + FLAGS + [HOST_SRC, "-o", exe], check=True)
    inp = S.random_inputs(3, 300, 300, seed=303)
    _, marked, windows = _run_pair_program(exe, inp, _search(inp, host=True), tmp_path)
    with capsys.disabled():
        print(f"\natan2f: largest deviation {int(dev_host.max())} f32 step(s) from the correctly rounded value over {n} normals "
              f"({int((dev_host > 0).sum())} differ); marked by the level's or theta's rule: {marked} of {windows} windows")


def test_header_declares_and_library_exports_the_three_entries():
    from plvs_amd import _lib
    with open(os.path.join(ROOT, "include", "plvs_hip.h")) as fh:
        header = fh.read()
    for name in ENTRIES[:2]:
        assert re.search(r"\bint " + name + r"\(const plvs_line_fuse_keyframe\* kfs, int n_kfs, const plvs_fuse_lines\* L", header), name
    assert re.search(r"\bint plvs_hip_fuse_search_points_and_lines\(const plvs_fuse_keyframe\* point_kfs", header)
    for name in ENTRIES:
        assert hasattr(_lib.lib, name), name
    assert "typedef struct plvs_line_fuse_keyframe" in header and "typedef struct plvs_fuse_lines" in header
    for code, name in enumerate(R.REACHED):
        assert re.search(r"#define PLVS_LINE_FUSE_" + name.upper() + r" " + str(code) + r"\b", header), name
    assert _lib.lib.plvs_hip_abi_version() == 1
    with open(os.path.join(ROOT, "include", "plvs_hip.hpp")) as fh:
        hpp = fh.read()
    assert "FuseSearchPointsAndLines" in hpp and "plvs_hip_line_fuse_search_host" in hpp


def _searcher(host):
    def search(kfs, lines, skip):
        return _search(dict(kfs=kfs, lines=lines, skip=skip, th=S.TH), host=host, skip=skip)["best_idx"]
    return search


def _check_replay(batch_host):
    inp = P.replay_inputs()
    host = _searcher(True)
    want = P.sequential(inp, host)
    log = []
    got = P.replayed(inp, host, batch_search=_searcher(batch_host), log=log)
    assert got.state() == want.state()
    M = inp["M"]
    assert any(loser < M for loser, _ in want.replacements), "no current line was replaced by an older one"
    assert any(loser >= M for loser, _ in want.replacements), "no older line was replaced by a current one"
    assert any(stale != live for _, _, stale, live in log), "no dirty line whose stale candidate differs from its live one"
    # and the rule is needed: the batch's candidates with the live re-tests but without the re-query of dirty lines end elsewhere
    assert P.replayed(inp, host, batch_search=_searcher(batch_host), requery=False).state() != want.state()


def test_replay_of_one_batched_search_equals_the_sequential_loop():
    _check_replay(batch_host=True)


# ---------------------------------------------------------------------------------------------------------------- GPU

@pytest.mark.gpu
def test_device_golden_scenario(scenario, golden, restated):
    out = _search(scenario, host=False)
    _same(out, golden)
    assert out["stats"].tolist() == [int(restated[0]["ambiguous"].sum()), _window_pairs(golden), 1]


@pytest.mark.gpu
@pytest.mark.parametrize("n_kfs", [1, 3])
@pytest.mark.parametrize("m", [1, 3, 4, 5, 63, 64, 65, 257])
def test_device_block_edge_sizes(m, n_kfs):
    """Four pairs per workgroup: 3 / 4 / 5 straddle it."""
    inp = S.random_inputs(n_kfs, m, 120, seed=m, empty_kf=1 if n_kfs == 3 else None)
    want = _search(inp, host=True)
    out = _search(inp, host=False)
    _same(out, want)
    assert out["stats"][1] == want["stats"][1] and out["stats"][2] == 1


@pytest.mark.gpu
def test_device_crowd_turns_the_stride_loop(crowd, golden, facts):
    g = R.grid_of(crowd["kfs"][0])
    assert len(g[1]) > 128 and facts["facts"]["crowd_counts"]["beyond_member_64"] == 8     # more than two strides; the best beyond member 64
    _same(_search(crowd, host=False), {k: golden["crowd_" + k] for k in OUTPUTS})


@pytest.mark.gpu
def test_device_ambiguous_pairs_go_through_the_host(ambiguous):
    inp, want, c = ambiguous
    out, host = _search(inp, host=False), _search(inp, host=True)
    assert out["stats"][0] == int(want["ambiguous"].sum()) >= c["ambiguous_theta"] + 1
    _same(out, host)
    _same(out, want)


@pytest.mark.gpu
def test_device_refusals_launch_nothing(scenario):
    from plvs_amd import _lib
    from plvs_amd.linematcher import LineFuseKeyFrame, LineMatcher       # noqa: F401
    _refusals(scenario, host=False)
    # outputs untouched, nothing launched: the entry is called by hand with buffers of its own
    kfs, lines = S.views(scenario)
    bad = [kfs[0], dataclasses.replace(kfs[1], n_cameras=2), kfs[2]]
    from plvs_amd.linematcher import _LineFuseKeyFrameC
    arr = (_LineFuseKeyFrameC * 3)(*[kf.as_c() for kf in bad])
    lc = lines.as_c()
    K, M = 3, lc.m
    bi, bd, rc_, st = np.full((K, M), -7, np.int32), np.full((K, M), -7, np.int32), np.full((K, M), 255, np.uint8), np.full(3, -1, np.int32)
    f = _lib.lib.plvs_hip_line_fuse_search
    vp = ctypes.c_void_p
    f.argtypes = [vp, ctypes.c_int, vp, vp, ctypes.c_float, vp, vp, vp, vp, vp]
    assert f(arr, K, ctypes.byref(lc), None, 3.0, _lib.np_ptr(bi), _lib.np_ptr(bd), _lib.np_ptr(rc_), _lib.np_ptr(st), None) == _lib.PLVS_ERR_INVALID_ARG
    assert (bi == -7).all() and (bd == -7).all() and (rc_ == 255).all() and st.tolist() == [-1, -1, -1]
    # a theta interval wider than pi is found on the device: refused with the reason, no output written
    wide = _wide_theta(scenario)
    wk, wl = S.views(wide)
    arr = (_LineFuseKeyFrameC * 3)(*[kf.as_c() for kf in wk])
    wc = wl.as_c()
    sk = np.ascontiguousarray(wide["skip"], np.uint8)
    assert f(arr, K, ctypes.byref(wc), _lib.np_ptr(sk), 3.0, _lib.np_ptr(bi), _lib.np_ptr(bd), _lib.np_ptr(rc_), _lib.np_ptr(st), None) == _lib.PLVS_ERR_INVALID_ARG
    assert (bi == -7).all() and (bd == -7).all() and (rc_ == 255).all()


@pytest.mark.gpu
@pytest.mark.parametrize("shape", ["no_kfs", "no_lines", "no_key_lines", "all_skipped"])
def test_device_empty_shapes_launch_nothing(shape):
    inp = S.random_inputs(0 if shape == "no_kfs" else 2, 0 if shape == "no_lines" else 40, 0 if shape == "no_key_lines" else 60, seed=4)
    if shape == "all_skipped":
        inp["skip"] = np.ones_like(inp["skip"])
    out = _search(inp, host=False)
    assert out["stats"][2] == 0 and out["stats"][0] == 0
    if shape in ("no_key_lines", "all_skipped"):
        want = R.fuse_search(inp["kfs"], inp["lines"], inp["skip"], inp["th"])
        _same(out, want)
        assert (out["reached"] == R.SKIPPED).all() if shape == "all_skipped" else (out["reached"] <= R.EMPTY_WINDOW).all()
    else:
        assert out["best_idx"].size == 0


@pytest.mark.gpu
def test_device_replay_equals_the_sequential_loop():
    _check_replay(batch_host=False)


@pytest.mark.gpu
def test_combined_entry_equals_the_two_entries_after_one_wait(scenario, golden):
    """plvs_hip_fuse_search_points_and_lines on the two golden scenarios: every output of either kind equals the separate entry's
    (and the reference's recorded run), with two launches and one wait; with either kind absent it is the other entry."""
    from plvs_amd.linematcher import FuseSearchPointsAndLines
    from plvs_amd.orbmatcher import ORBmatcher
    from tests import orb_fuse_scenario as PS
    pin = PS.inputs()
    pk, pp = PS.views(pin)
    lk, ll = S.views(scenario)
    want_p = ORBmatcher().FuseSearch(pk, pp, pin["th"], pin["skip"])
    want_l = _search(scenario, host=False)
    _same(want_l, golden)
    p, l, stats = FuseSearchPointsAndLines(pk, pp, pin["th"], pin["skip"], lk, ll, scenario["th"], scenario["skip"])
    _same(p, want_p, what="points ")
    _same(l, want_l, what="lines ")
    assert p["stats"].tolist() == want_p["stats"].tolist() and l["stats"].tolist() == want_l["stats"].tolist()
    assert stats.tolist() == [2, 1]
    p, l, stats = FuseSearchPointsAndLines(pk, pp, pin["th"], pin["skip"])
    assert l is None and stats.tolist() == [1, 1]
    _same(p, want_p, what="points alone ")
    p, l, stats = FuseSearchPointsAndLines(line_key_frames=lk, lines=ll, th_lines=scenario["th"], skip_lines=scenario["skip"])
    assert p is None and stats.tolist() == [1, 1]
    _same(l, want_l, what="lines alone ")
