"""The Sim3 Fuse searches of LoopClosing::SearchAndFuse over resident key frames (plvs_hip_orb_loop_fuse_search_kf,
plvs_hip_line_loop_fuse_search_kf, plvs_hip_loop_fuse_search_points_and_lines_kf and the two _kf_host entries) against the compiled
reference's recorded run (tests/golden/loop_fuse_reference.npz, scripts/make_loop_fuse_golden.py) and, at other sizes, against the
restatement that the golden pins (tests/loop_fuse_restatement.py).  Every comparison is for equality."""
import ctypes
import json
import os
import re
import subprocess

import numpy as np
import pytest

from tests import line_fuse_restatement as LR
from tests import loop_fuse_replay as RP
from tests import loop_fuse_restatement as R
from tests import loop_fuse_scenario as S
from tests import orb_fuse_restatement as PR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "loop_fuse_reference.npz")
FACTS = os.path.join(ROOT, "tests", "golden", "loop_fuse_reference_facts.json")
OUTPUTS = ("best_idx", "best_dist", "reached")
ENTRIES = ("plvs_hip_orb_loop_fuse_search_kf", "plvs_hip_line_loop_fuse_search_kf", "plvs_hip_loop_fuse_search_points_and_lines_kf",
           "plvs_hip_orb_loop_fuse_search_kf_host", "plvs_hip_line_loop_fuse_search_kf_host")


@pytest.fixture(scope="module", autouse=True)
def entries_exist():
    """Every test here is about these entries: without them the first missing symbol fails it."""
    from plvs_amd import _lib
    for name in ENTRIES + ("plvs_hip_loop_fuse_test_layout",):
        assert hasattr(_lib.lib, name), name


def same(out, want, what=""):
    for k in OUTPUTS:
        a, b = np.asarray(out[k]), np.asarray(want[k])
        assert a.shape == b.shape and (a == b).all(), f"{what}{k} differs at {np.argwhere(a != b)[:8].tolist()}"


@pytest.fixture(scope="module")
def golden():
    g = dict(np.load(GOLDEN))
    for pre, cand in (("point_", PR.CANDIDATE), ("point_crowd_", PR.CANDIDATE), ("line_", LR.CANDIDATE), ("line_crowd_", LR.CANDIDATE)):
        c = g[pre + "reached"] == cand      # the entries' outputs from the recorded bestIdx / bestDist
        g[pre + "best_idx"] = np.where(c, g[pre + "raw_best_idx"], -1).astype(np.int32)
        g[pre + "best_dist"] = np.where(c, g[pre + "raw_best_dist"], -1).astype(np.int32)
    return g


def part(golden, pre):
    return {k: golden[pre + k] for k in OUTPUTS}


@pytest.fixture(scope="module")
def facts():
    with open(FACTS) as fh:
        return json.load(fh)


@pytest.fixture(scope="module")
def sets():
    return dict(point_=S.point_inputs(), point_crowd_=S.crowd_point_inputs(), line_=S.line_inputs(), line_crowd_=S.crowd_line_inputs())


def restate(inp, facts=None):
    d = facts["facts"]["double_overloads"] if facts else dict(point_log=0, line_log=0, atan2=0)
    if "points" in inp:
        return R.point_search(inp["kfs"], inp["points"], inp["skip"], inp["th"], None, bool(d["point_log"]))
    return R.line_search(inp["kfs"], inp["lines"], inp["skip"], inp["th"], None, bool(d["line_log"]), bool(d["atan2"]))


def search(inp, host, layout=None, **kw):
    """The single-kind entry over handles made for the call (host: host-only handles and the _kf_host entry)."""
    from plvs_amd.keyframe import line_loop_fuse_search_kf, loop_fuse_search_kf, loop_fuse_test_layout
    points = "points" in inp
    with S.Handles(points_inp=inp if points else None, lines_inp=None if points else inp, host_only=host) as h:
        if layout is not None:
            loop_fuse_test_layout(layout)
        try:
            f, items = (loop_fuse_search_kf, h.points) if points else (line_loop_fuse_search_kf, h.lines)
            return f(h.kfs, h.poses, items, inp["th"], inp["skip"], host=host, **kw)
        finally:
            if layout is not None:
                loop_fuse_test_layout(0)


def windows(r, first):
    return int((np.asarray(r["reached"]) >= first).sum())


# ---------------------------------------------------------------------------------------------------------------- the pin

def test_scenario_digests_match_the_golden(sets, golden, facts):
    for pre, inp in sets.items():
        d = S.digest(inp)
        assert d == str(golden[pre + "inputs_digest"]) == facts["digests"][pre + "inputs"], pre


def test_restatement_equals_the_golden(sets, golden, facts):
    for pre, inp in sets.items():
        rest = restate(inp, facts)
        same(rest, part(golden, pre), pre)
        for k in ("raw_best_dist", "n_dist") + (("u", "v") if "points" in inp else ("level", "n_proj", "proj")):
            assert rest[k].tobytes() == golden[pre + k].tobytes(), pre + k


def test_golden_run_takes_every_stage_and_every_placed_case(sets, golden, facts):
    f = facts["facts"]
    for code, name in enumerate(PR.REACHED):
        assert (golden["point_reached"] == code).any() and f["point_counts"][name] >= 1, name
    for code, name in enumerate(LR.REACHED):
        if name != "degenerate":               # undefined in the reference: not in its run
            assert (golden["line_reached"] == code).any() and f["line_counts"][name] >= 1, name
    for k in R.POINT_SUB_FACTS:
        assert f["point_counts"][k] >= 1 or k == "dist3d_zero", k
    for k in ("taken_where_kl_level_sigma_drops", "taken_where_right_gate_drops", "split_at_minus_half_pi", "split_at_plus_half_pi",
              "tie_winner_in_wrapped_part_higher_index", "clipped_column_0", "clipped_column_159", "best_dist_60", "best_dist_61"):
        assert f["line_counts"][k] >= 1, k
    assert f["ambiguous_counts"]["points"] >= 1 and f["ambiguous_counts"]["line_level"] >= 1 and f["ambiguous_counts"]["line_theta"] >= 1
    assert f["point_crowd_counts"]["tie_winner_not_lowest_index"] >= 1 and f["line_crowd_counts"]["beyond_member_64"] >= 1
    # what only the Sim3 overloads take: candidates in the golden, with the placed member, and rejected by the SE3 restatement
    w, inp = sets["point_"]["where"], sets["point_"]
    se3 = PR.fuse_search([R.point_kf(kf) for kf in inp["kfs"]], inp["points"], inp["skip"], inp["th"], None, bool(f["double_overloads"]["point_log"]))
    for name, member in zip(("chi2_far", "chi2_stereo_far"), w["chi2_members"]):
        i = w[name][0]
        assert golden["point_reached"][0, i] == PR.CANDIDATE and golden["point_best_idx"][0, i] == member and se3["reached"][0, i] == PR.NO_CANDIDATE
    for name in ("mono_gate", "stereo_gate", "u_right_zero"):
        assert golden["point_reached"][0, w[name][0]] == PR.CANDIDATE and se3["reached"][0, w[name][0]] == PR.NO_CANDIDATE, name
    ja, jb = w["tie_indices"]
    assert ja > jb and golden["point_best_idx"][0, w["tie"][0]] == ja
    assert np.isnan(golden["point_u"][2, w["z_zero_nan"][0]]) and np.isinf(golden["point_u"][2, w["z_zero_inf"][0]])
    assert golden["point_reached"][0, w["above_th_low"][0]] == PR.ABOVE_TH_LOW
    lw, linp = sets["line_"]["where"], sets["line_"]
    lse3 = LR.fuse_search([R.line_kf(kf) for kf in linp["kfs"]], linp["lines"], linp["skip"], linp["th"], None,
                          bool(f["double_overloads"]["line_log"]), bool(f["double_overloads"]["atan2"]))
    for name, member in zip(("sigma_level", "right_far"), lw["sim3_members"]):
        i = lw[name][0]
        assert golden["line_reached"][0, i] == LR.CANDIDATE and golden["line_best_idx"][0, i] == member and lse3["reached"][0, i] == LR.NO_CANDIDATE
    assert [s["scale"] for s in inp["kfs"]] == pytest.approx([1.7, 0.6, 4.0]) and len(inp["kfs"]) >= 3


# ---------------------------------------------------------------------------------------------------------------- the host entries

def test_host_entries_equal_the_golden(sets, golden):
    for pre, inp in sets.items():
        out = search(inp, host=True)
        same(out, part(golden, pre), pre)
        first = PR.EMPTY_WINDOW if "points" in inp else LR.EMPTY_WINDOW
        assert out["stats"].tolist() == [0, windows(part(golden, pre), first), 0, 0], pre


SHAPES = [(3, 300, 300, None), (2, 65, 100, 1), (1, 1, 1, None), (3, 257, 40, None)]


@pytest.fixture(scope="module")
def random_sets():
    out = {}
    for K, M, N, empty in SHAPES:
        out[("points", K, M)] = S.random_point_inputs(K, M, N, seed=K + M, empty_kf=empty)
        out[("lines", K, M)] = S.random_line_inputs(K, M, N, seed=K + M, empty_kf=empty)
    return {k: (inp, restate(inp)) for k, inp in out.items()}


@pytest.mark.parametrize("kind", ["points", "lines"])
@pytest.mark.parametrize("shape", SHAPES)
def test_host_entries_equal_the_restatement_at_other_sizes(random_sets, kind, shape):
    inp, want = random_sets[(kind, shape[0], shape[1])]
    same(search(inp, host=True), want)


def test_host_entries_take_the_ambiguous_through_the_hosts_libm():
    for inp in (S.ambiguous_point_inputs(), S.ambiguous_line_inputs()):
        want = restate(inp)
        assert want["ambiguous"].sum() >= 12
        same(search(inp, host=True), want)


def test_entries_refuse_before_any_device_call(sets):
    from plvs_amd import _lib
    from plvs_amd.keyframe import (_lists, line_loop_fuse_search_kf, loop_fuse_search_kf, loop_fuse_search_points_and_lines_kf)
    pinp, linp = sets["point_"], sets["line_"]
    with S.Handles(points_inp=pinp, host_only=True) as P, S.Handles(lines_inp=linp, host_only=True) as L:
        def refused(what, f, *a, **kw):
            with pytest.raises(_lib.PlvsHipError) as e:
                f(*a, **kw)
            assert e.value.code == _lib.PLVS_ERR_INVALID_ARG and what in str(e.value), str(e.value)

        for host in (True, False):
            refused("null key-frame handle", loop_fuse_search_kf, [P.kfs[0], None, P.kfs[2]], P.poses, P.points, host=host)
            refused("null key-frame handle", line_loop_fuse_search_kf, [None] + L.kfs[1:], L.poses, L.lines, host=host)
            refused("without a line side", line_loop_fuse_search_kf, P.kfs, P.poses, L.lines, host=host)
            refused("without a point side", loop_fuse_search_kf, L.kfs, L.poses, P.points, host=host)
            refused("th outside", loop_fuse_search_kf, P.kfs, P.poses, P.points, th=-1.0, host=host)
            refused("th outside", line_loop_fuse_search_kf, L.kfs, L.poses, L.lines, th=2.0e6, host=host)
            refused("null output", line_loop_fuse_search_kf, L.kfs, L.poses, L.lines, host=host, outputs=False)
            refused("null output", loop_fuse_search_kf, P.kfs, P.poses, P.points, host=host, outputs=False)
        # a host-only handle in a device entry: refused before any HIP call (this machine may have no device to call)
        refused("PLVS_KEYFRAME_HOST_ONLY", loop_fuse_search_kf, P.kfs, P.poses, P.points)
        refused("PLVS_KEYFRAME_HOST_ONLY", line_loop_fuse_search_kf, L.kfs, L.poses, L.lines)
        refused("PLVS_KEYFRAME_HOST_ONLY", loop_fuse_search_points_and_lines_kf, P.kfs, P.poses, points=P.points)
        refused("neither points nor lines", loop_fuse_search_points_and_lines_kf, P.kfs, P.poses)
        # a NULL pose list, and nothing written by a refused call: through the C entries
        vp = ctypes.c_void_p
        K, hs, ps = _lists(P.kfs, P.poses)
        pc = P.points.as_c()
        for name, tail in (("plvs_hip_orb_loop_fuse_search_kf", [None]), ("plvs_hip_orb_loop_fuse_search_kf_host", [])):
            f = getattr(_lib.lib, name)
            f.argtypes = [vp, vp, ctypes.c_int, vp, vp, ctypes.c_float, vp, vp, vp, vp] + [vp] * len(tail)
            for poses, th, what in ((None, 4.0, "null poses"), (ps, -1.0, "th outside")):
                out, dist, st = np.full((3, pc.m), -7, np.int32), np.full((3, pc.m), -7, np.int32), np.full(4, -1, np.int32)
                assert f(hs, poses, K, ctypes.byref(pc), None, th, _lib.np_ptr(out), _lib.np_ptr(dist), None, _lib.np_ptr(st), *tail) == _lib.PLVS_ERR_INVALID_ARG
                assert what in _lib.lib.plvs_hip_last_error().decode()
                assert (out == -7).all() and (dist == -7).all() and st.tolist() == [-1] * 4


def test_the_wide_theta_interval_refuses_the_line_call(sets):
    from plvs_amd import _lib
    kfs = [dict(kf) for kf in sets["line_"]["kfs"]]
    kfs[1]["scale_factors"] = np.array([1.0, 10.0, 1.44], np.float32)      # deltaTheta = 100 degrees at level 1
    with pytest.raises(_lib.PlvsHipError) as e:
        search(dict(sets["line_"], kfs=kfs), host=True)
    assert e.value.code == _lib.PLVS_ERR_INVALID_ARG and "theta" in str(e.value)


def test_header_declares_and_library_exports_the_loop_entries():
    from plvs_amd import _lib, keyframe
    with open(os.path.join(ROOT, "include", "plvs_hip.h")) as fh:
        header = fh.read()
    for name in ENTRIES:
        assert re.search(r"\bint " + name + r"\(const plvs_keyframe\* const\* kfs, const plvs_keyframe_sim3_pose\* sim3_poses, int n_kfs", header), name
        assert hasattr(_lib.lib, name), name
    assert re.search(r"\bvoid plvs_hip_loop_fuse_test_layout\(int mode\);", header) and hasattr(_lib.lib, "plvs_hip_loop_fuse_test_layout")
    m = re.search(r"typedef struct plvs_keyframe_sim3_pose \{(.*?)\} plvs_keyframe_sim3_pose;", header, re.S)
    assert re.findall(r"float (\w+)\[(\d+)\];", m.group(1)) == [("q_cw", "4"), ("Rcw", "9"), ("tcw", "3"), ("Ow_points", "3"), ("Ow_lines", "3")]
    assert ctypes.sizeof(keyframe._Sim3PoseC) == 4 * 22
    assert _lib.lib.plvs_hip_abi_version() == 1
    with open(os.path.join(ROOT, "include", "plvs_hip.hpp")) as fh:
        hpp = fh.read()
    assert hpp.count("inline int LoopFuseSearch(") == 2 and "inline int LoopFuseSearchPointsAndLines(" in hpp
    for name in ("loop_fuse_search_kf", "line_loop_fuse_search_kf", "loop_fuse_search_points_and_lines_kf", "loop_fuse_test_layout"):
        assert callable(getattr(keyframe, name)), name


# ---------------------------------------------------------------------------------------------------------------- the pair headers alone

FLAGS = ["-std=c++14", "-ffp-contract=off", "-Wall", "-Wextra", "-Werror"]
PAIR_SRC = os.path.join(ROOT, "tests", "host", "loop_fuse_pair_host.cpp")


def _check_pair_program(exe, sets, golden, tmp_path, env=None):
    from tests.test_line_fuse import _write_pair_input as write_lines
    from tests.test_orb_fuse import _write_pair_input as write_points
    errors = ""
    for pre, inp in sets.items():
        kind = "points" if "points" in inp else "lines"
        path = str(tmp_path / (pre + "input.bin"))
        (write_points if kind == "points" else write_lines)(path, inp)
        r = subprocess.run([exe, kind, path], capture_output=True, text=True, env=env)
        assert r.returncode == 0 and "loop_fuse_pair ok" in r.stdout, r.stderr + r.stdout[-500:]
        got = np.array([[int(c) for c in ln.split()[1:]] for ln in r.stdout.splitlines() if ln.startswith("pair ")], np.int64)
        want = np.stack([golden[pre + k].reshape(-1).astype(np.int64) for k in OUTPUTS], 1)
        assert got.shape == want.shape and (got == want).all(), (pre, np.argwhere(got != want)[:8])
        errors += r.stderr
    return errors


@pytest.mark.parametrize("compiler", ["g++", "/opt/rocm/llvm/bin/clang++"])
def test_pair_headers_alone_reproduce_the_reference(sets, golden, tmp_path, compiler):
    """fuse_pair.hpp and line_fuse_pair.hpp — the text the kernels compile — with the Sim3 gate, as a stand-alone host program under g++
    and ROCm's clang."""
    if not os.path.exists(compiler) and compiler != "g++":
        pytest.fail(f"{compiler} is missing")
    exe = str(tmp_path / "loop_fuse_pair_host")
    subprocess.run([compiler, "-O2"] + FLAGS + [PAIR_SRC, "-o", exe], check=True)
    _check_pair_program(exe, sets, golden, tmp_path)


def test_pair_headers_under_the_sanitizers(sets, golden, tmp_path):
    exe = str(tmp_path / "loop_fuse_pair_host_san")
    subprocess.run(["g++", "-O1", "-g"] + FLAGS + ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", PAIR_SRC, "-o", exe], check=True)
    err = _check_pair_program(exe, sets, golden, tmp_path, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1"))
    assert "ERROR: AddressSanitizer" not in err and "runtime error" not in err, err


# ---------------------------------------------------------------------------------------------------------------- the replay

def _check_replay(batch_host):
    inp = RP.replay_inputs()
    host, batch = RP.Searcher(True), RP.Searcher(batch_host)
    try:
        want = RP.sequential(inp, host)
        log = []
        got = RP.replayed(inp, host, batch_search=batch, log=log)
        assert got.state() == want.state()
        M = inp["M"]
        assert any(loser >= M for loser, _ in want.replacements), "no older point was replaced by a loop point"
        # two loop points chose the same empty slot of key frame 0: the first took it, the second replaced the first
        assert (1, 2) in want.replacements and want.bad[1] and not want.bad[2]
        assert any(stale != live for _, _, stale, live in log), "no dirty point whose stale candidate differs from its live one"
        # and the rule is needed: the batch's candidates with the live re-tests but without the re-query of dirty points end elsewhere
        assert RP.replayed(inp, host, batch_search=batch, requery=False).state() != want.state()
    finally:
        host.close()
        batch.close()


def test_replay_of_one_batched_search_equals_the_sequential_loops():
    _check_replay(batch_host=True)


# ---------------------------------------------------------------------------------------------------------------- GPU

@pytest.mark.gpu
@pytest.mark.parametrize("layout", [0, 1])
def test_device_golden_scenario_and_crowd_on_both_layouts(sets, golden, layout):
    for pre, inp in sets.items():
        out = search(inp, host=False, layout=layout)
        same(out, part(golden, pre), f"layout {layout} {pre}")
        first = PR.EMPTY_WINDOW if "points" in inp else LR.EMPTY_WINDOW
        assert out["stats"][1:3].tolist() == [windows(part(golden, pre), first), 1], pre
        assert out["stats"][3] > 0


@pytest.mark.gpu
def test_device_combined_entry_equals_the_two_single_entries(sets):
    from plvs_amd.keyframe import line_loop_fuse_search_kf, loop_fuse_search_kf, loop_fuse_search_points_and_lines_kf
    pinp, linp = sets["point_"], sets["line_"]
    with S.Handles(points_inp=pinp, lines_inp=linp) as h:
        p1 = loop_fuse_search_kf(h.kfs, h.poses, h.points, S.TH, pinp["skip"])
        l1 = line_loop_fuse_search_kf(h.kfs, h.poses, h.lines, S.TH, linp["skip"])
        p2, l2, stats = loop_fuse_search_points_and_lines_kf(h.kfs, h.poses, h.points, S.TH, pinp["skip"], h.lines, S.TH, linp["skip"])
        same(p2, p1, "points ")
        same(l2, l1, "lines ")
        assert p2["stats"].tolist() == p1["stats"].tolist() and l2["stats"].tolist() == l1["stats"].tolist()
        assert stats.tolist() == [2, 1, int(p1["stats"][3] + l1["stats"][3])]
        # the line side alone is the line entry
        none, l3, stats = loop_fuse_search_points_and_lines_kf(h.kfs, h.poses, lines=h.lines, th_lines=S.TH, skip_lines=linp["skip"])
        assert none is None and stats.tolist() == [1, 1, int(l1["stats"][3])]
        same(l3, l1)
    # the line poses differ from the point set's own: the point results are another search's, the line results the golden's
    same(l1, restate(linp), "lines ")


@pytest.mark.gpu
@pytest.mark.parametrize("K", [1, 3])
@pytest.mark.parametrize("M", [1, 63, 64, 65, 255, 256, 257, 513])
def test_device_sieve_edges(K, M):
    inp = S.random_point_inputs(K, M, 80, seed=100 * K + M)
    want = restate(inp)
    for layout in (0, 1):
        same(search(inp, host=False, layout=layout), want, f"layout {layout} ")


def _tiles():
    """Two key frames x 1025 points, every point a survivor of the projection's tests in its own key frame until its normal is turned
    away: tile 0 without a survivor, tile 1 with 256, tile 2 with one in lane 63 of wave 3, tile 3 with wave 3 alone, tile 4 with
    its one valid pair."""
    from tests import orb_fuse_scenario as PS
    rng = np.random.default_rng(S.SEED + 9)
    kfs = [PS._random_kf(rng, q, t, 120, PS.H - 12.0) for q, t in PS._poses(2)]
    pts = []
    PS._matching_points(rng, kfs[:1], 1025, pts)
    points = PS._pack(pts)
    keep = np.zeros(1025, bool)
    keep[256:512] = True
    keep[512 + 255] = True
    keep[768 + 192:1024] = True
    keep[1024] = True
    points["normal"][~keep] *= -1
    return dict(kfs=S._as("points", PS._public(kfs), S.SCALES), points=points, skip=None, th=S.TH, where={}), keep


@pytest.mark.gpu
def test_device_constructed_tiles():
    inp, keep = _tiles()
    want = restate(inp)
    assert ((want["reached"][0] >= PR.EMPTY_WINDOW) == keep).all(), "the tiles are not what they were built to be"
    for layout in (0, 1):
        out = search(inp, host=False, layout=layout)
        same(out, want, f"layout {layout} ")
        assert out["stats"][2] == 1


@pytest.mark.gpu
def test_device_key_frames_without_features():
    for inp in (S.random_point_inputs(3, 130, 60, seed=21, empty_kf=1), S.random_line_inputs(3, 70, 60, seed=21, empty_kf=0)):
        want = restate(inp)
        out = search(inp, host=False)
        same(out, want)
        assert out["stats"][2] == 1


@pytest.mark.gpu
def test_device_launch_free_shapes():
    from plvs_amd.keyframe import line_loop_fuse_search_kf, loop_fuse_search_kf
    pinp, linp = S.random_point_inputs(2, 40, 50, seed=31), S.random_line_inputs(2, 40, 50, seed=31)
    for inp in (pinp, linp):
        out = search(dict(inp, skip=np.ones_like(inp["skip"])), host=False)
        assert out["stats"].tolist() == [0, 0, 0, 0] and (out["reached"] == 0).all() and (out["best_idx"] == -1).all()
        empty = dict(inp, kfs=[dict(kf, **({"x": kf["x"][:0], "y": kf["y"][:0], "octave": kf["octave"][:0], "u_right": kf["u_right"][:0],
                                            "desc": kf["desc"][:0]} if "points" in inp else
                                           {"kl": kf["kl"][:0], "desc": kf["desc"][:0], "u_right_start": None, "u_right_end": None}))
                               for kf in inp["kfs"]])
        out = search(empty, host=False)
        same(out, restate(empty))
        assert out["stats"][2:].tolist() == [0, 0]
    with S.Handles(points_inp=pinp, lines_inp=linp) as h:
        out = loop_fuse_search_kf([], [], h.points, S.TH, None)
        assert out["best_idx"].shape == (0, 40) and out["stats"].tolist() == [0, 0, 0, 0]
        out = line_loop_fuse_search_kf([], [], h.lines, S.TH, None)
        assert out["best_idx"].shape == (0, 40) and out["stats"].tolist() == [0, 0, 0, 0]
        from plvs_amd.linematcher import FuseLines
        from plvs_amd.orbmatcher import FusePoints
        z3, z1, zd = np.zeros((0, 3), np.float32), np.zeros(0, np.float32), np.zeros((0, 32), np.uint8)
        out = loop_fuse_search_kf(h.kfs, h.poses, FusePoints(z3, z3, z1, z1, zd), S.TH, None)
        assert out["best_idx"].shape == (2, 0) and out["stats"].tolist() == [0, 0, 0, 0]
        out = line_loop_fuse_search_kf(h.kfs, h.poses, FuseLines(z3, z3, z3, z1, zd), S.TH, None)
        assert out["best_idx"].shape == (2, 0) and out["stats"].tolist() == [0, 0, 0, 0]


@pytest.mark.gpu
def test_device_ambiguous_pairs_come_back_as_the_hosts():
    for inp in (S.ambiguous_point_inputs(), S.ambiguous_line_inputs()):
        want = restate(inp)
        host = search(inp, host=True)
        for layout in ((0, 1) if "points" in inp else (None,)):
            out = search(inp, host=False, layout=layout)
            same(out, host)
            same(out, want)
            assert out["stats"][0] >= 12 and out["stats"][0] <= int(want["ambiguous"].sum())


@pytest.mark.gpu
def test_device_refusals_launch_nothing_and_write_nothing(sets):
    from plvs_amd import _lib
    from plvs_amd.keyframe import _lists
    pinp = sets["point_"]
    vp = ctypes.c_void_p
    with S.Handles(points_inp=pinp) as P:
        K, hs, ps = _lists(P.kfs, P.poses)
        bad = (vp * K)(*[None if k == 1 else P.kfs[k].handle for k in range(K)])
        pc = P.points.as_c()
        f = _lib.lib.plvs_hip_orb_loop_fuse_search_kf
        f.argtypes = [vp, vp, ctypes.c_int, vp, vp, ctypes.c_float, vp, vp, vp, vp, vp]
        for handles, poses, th, idx_null in ((bad, ps, 4.0, False), (hs, None, 4.0, False), (hs, ps, -1.0, False), (hs, ps, 4.0, True)):
            out, dist, st = np.full((K, pc.m), -7, np.int32), np.full((K, pc.m), -7, np.int32), np.full(4, -1, np.int32)
            rc = f(handles, poses, K, ctypes.byref(pc), None, th, None if idx_null else _lib.np_ptr(out), _lib.np_ptr(dist), None, _lib.np_ptr(st), None)
            assert rc == _lib.PLVS_ERR_INVALID_ARG and (out == -7).all() and (dist == -7).all() and st.tolist() == [-1] * 4


@pytest.mark.gpu
def test_device_the_same_handle_twice_with_two_poses(sets):
    from plvs_amd.keyframe import loop_fuse_search_kf
    inp = sets["point_"]
    want = restate(dict(inp, kfs=[inp["kfs"][0], dict(inp["kfs"][0], **{k: inp["kfs"][1][k] for k in ("q_cw", "Rcw", "tcw", "Ow_points", "Ow_lines")})],
                        skip=None))
    with S.Handles(points_inp=inp) as h:
        out = loop_fuse_search_kf([h.kfs[0], h.kfs[0]], [h.poses[0], h.poses[1]], h.points, S.TH, None)
    same(out, want)
    assert (want["reached"][0] != want["reached"][1]).any()


@pytest.mark.gpu
def test_device_replay_equals_the_sequential_loops():
    _check_replay(batch_host=False)
