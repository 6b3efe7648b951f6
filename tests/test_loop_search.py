"""The loop-closing SearchByProjection(pKF, Scw, ...) searches over resident key frames (plvs_hip_orb_loop_search_by_projection_kf,
plvs_hip_line_loop_search_by_projection_kf, plvs_hip_loop_search_by_projection_points_and_lines_kf and the two _kf_host entries)
against the compiled reference's recorded run (tests/golden/loop_search_reference.npz, scripts/make_loop_search_golden.py) and, at
other sizes, against the restatement that the golden pins (tests/loop_search_restatement.py).  Every comparison is for equality."""
import ctypes
import json
import os
import re
import struct
import subprocess

import numpy as np
import pytest

from tests import line_fuse_restatement as LR
from tests import loop_search_restatement as R
from tests import loop_search_scenario as S
from tests import orb_fuse_restatement as PR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "loop_search_reference.npz")
FACTS = os.path.join(ROOT, "tests", "golden", "loop_search_reference_facts.json")
OUTPUTS = ("match_idx", "match_dist", "reached", "nmatches")
ENTRIES = ("plvs_hip_orb_loop_search_by_projection_kf", "plvs_hip_line_loop_search_by_projection_kf",
           "plvs_hip_loop_search_by_projection_points_and_lines_kf", "plvs_hip_orb_loop_search_by_projection_kf_host",
           "plvs_hip_line_loop_search_by_projection_kf_host")
L = R.LIST_LEN


@pytest.fixture(scope="module", autouse=True)
def entries_exist():
    """Every test here is about these entries: without them the first missing symbol fails it."""
    from plvs_amd import _lib
    for name in ENTRIES:
        assert hasattr(_lib.lib, name), name


def same(out, want, what=""):
    for k in OUTPUTS:
        a, b = np.asarray(out[k]), np.asarray(want[k])
        assert a.shape == b.shape and (a == b).all(), f"{what}{k} differs at {np.argwhere(a != b)[:8].tolist()}"


@pytest.fixture(scope="module")
def facts():
    with open(FACTS) as fh:
        return json.load(fh)


@pytest.fixture(scope="module")
def sets():
    return dict(point=S.point_inputs(), point_crowd=S.crowd_point_inputs(), line=S.line_inputs(), line_crowd=S.crowd_line_inputs())


def runs_of(inp):
    """(run name, projection or None, ratio) of a set's kind."""
    return S.RUNS if "points" in inp else tuple((name, None, ratio) for name, _, ratio in S.LINE_RUNS)


@pytest.fixture(scope="module")
def golden():
    g = dict(np.load(GOLDEN))
    for key in [k for k in g if k.endswith("_raw_best_dist")]:
        pre = key[:-len("raw_best_dist")]
        g[pre + "match_dist"] = np.where(g[pre + "match_idx"] >= 0, g[key], -1).astype(np.int32)      # the entries' output
    return g


def part(golden, sname, run):
    return {k: golden[f"{sname}_{run}_{k}"] for k in OUTPUTS}


def restate(inp, projection, ratio, facts=None):
    d = facts["facts"]["double_overloads"] if facts else dict(point_log=0, line_log=0, atan2=0)
    if "points" in inp:
        return R.point_search(inp["kfs"], inp["points"], inp["skip"], inp["occupied"], inp["th"], ratio, projection, None, bool(d["point_log"]))
    return R.line_search(inp["kfs"], inp["lines"], inp["skip"], inp["occupied"], inp["th"], ratio, None, bool(d["line_log"]), bool(d["atan2"]))


def search(inp, projection, ratio, host, handles=None, **kw):
    """The single-kind entry over handles made for the call (host: host-only handles and the _kf_host entry)."""
    from plvs_amd.keyframe import line_loop_search_by_projection_kf, loop_search_by_projection_kf
    points = "points" in inp

    def call(h):
        if points:
            return loop_search_by_projection_kf(h.kfs, h.poses, h.points, inp["th"], ratio, projection, inp["skip"], inp["occupied"], host=host, **kw)
        return line_loop_search_by_projection_kf(h.kfs, h.poses, h.lines, inp["th"], ratio, inp["skip"], inp["occupied"], host=host, **kw)

    if handles is not None:
        return call(handles)
    with S.Handles(points_inp=inp if points else None, lines_inp=None if points else inp, host_only=host) as h:
        return call(h)


def windows(r, inp):
    return int((np.asarray(r["reached"]) >= (PR.EMPTY_WINDOW if "points" in inp else LR.EMPTY_WINDOW)).sum())


# ---------------------------------------------------------------------------------------------------------------- the pin

def test_scenario_digests_match_the_golden(sets, golden, facts):
    for sname, inp in sets.items():
        d = S.digest(inp)
        assert d == str(golden[sname + "_inputs_digest"]) == facts["digests"][sname + "_inputs"], sname


def test_restatement_equals_the_golden(sets, golden, facts):
    for sname, inp in sets.items():
        for run, projection, ratio in runs_of(inp):
            rest = restate(inp, projection, ratio, facts)
            same(rest, part(golden, sname, run), f"{sname} {run} ")
            for k in ("raw_best_idx", "raw_best_dist", "n_dist", "level") + (("u", "v") if "points" in inp else ("n_proj", "proj")):
                assert rest[k].tobytes() == golden[f"{sname}_{run}_{k}"].tobytes(), (sname, run, k)


def test_golden_run_takes_every_stage_and_every_placed_case(sets, golden, facts):
    f = facts["facts"]
    assert f["list_len"] == L
    greedy = ("took_behind_a_claimed_best", "all_banded_claimed", "tie_winner_not_lowest_index", "occupied_would_have_won", "dist_at_cut",
              "dist_at_cut_plus_1")
    for run, _, _ in S.RUNS:
        for code, name in enumerate(PR.REACHED):
            assert (golden[f"point_{run}_reached"] == code).any() and f["counts"][f"point_{run}"][name] >= 1, (run, name)
        for k in greedy:
            assert f["counts"][f"point_{run}"][k] >= 1, (run, k)
        assert f["counts"][f"point_crowd_{run}"]["windows_over_list_len"] >= L + 2
    for run, _, _ in S.LINE_RUNS:
        for code, name in enumerate(LR.REACHED):
            if name != "degenerate":               # undefined in the reference: not in its run
                assert (golden[f"line_{run}_reached"] == code).any() and f["counts"][f"line_{run}"][name] >= 1, (run, name)
        for k in greedy:
            assert f["counts"][f"line_{run}"][k] >= 1, (run, k)
        assert f["counts"][f"line_crowd_{run}"]["windows_over_list_len"] >= L + 2
    assert f["ambiguous_counts"]["line_level"] >= 1 and f["ambiguous_counts"]["line_theta"] >= 1
    # the placed cases of the point set, on the recorded run
    w = sets["point"]["where"]
    cam, inv = (lambda k, name: int(golden[f"point_camera_r15_{k}"][0, w[name][0]])), (lambda k, name: int(golden[f"point_invz_r10_{k}"][0, w[name][0]]))
    for g in (cam, inv):
        assert g("match_idx", "second_best_first") == w["second_best_members"][0] and g("match_idx", "second_best") == w["second_best_members"][1]
        assert g("reached", "all_claimed") == PR.ABOVE_TH_LOW and g("raw_best_dist", "all_claimed") == 256
        assert g("match_idx", "occupied_wins") == w["occupied_members"][1]
        assert w["tie_indices"][0] > w["tie_indices"][1] and g("match_idx", "tie") == w["tie_indices"][0]
    assert [cam("reached", f"at_{b}") for b in (50, 51, 75, 76)] == [PR.CANDIDATE] * 3 + [PR.ABOVE_TH_LOW]
    assert [inv("reached", f"at_{b}") for b in (50, 51, 75, 76)] == [PR.CANDIDATE] + [PR.ABOVE_TH_LOW] * 3
    ua, ub = golden["point_camera_r15_u"][0, w["project_bit"][0]], golden["point_invz_r10_u"][0, w["project_bit"][0]]
    assert abs(int(ua.view(np.int32)) - int(ub.view(np.int32))) == 1, "the two projections do not differ in the last bit of u"
    assert {cam("reached", "project_bit"), inv("reached", "project_bit")} == {PR.CANDIDATE, PR.EMPTY_WINDOW}
    # and of the line set (its fourth key frame)
    lw = sets["line"]["where"]
    for run, want in (("kf0_r15", [LR.CANDIDATE] * 3 + [LR.ABOVE_TH_LOW]), ("kf1_r10", [LR.CANDIDATE] + [LR.ABOVE_TH_LOW] * 3)):
        g = lambda k, name, kf=3: int(golden[f"line_{run}_{k}"][kf, lw[name][0]])
        assert [g("reached", f"at_{b}") for b in (60, 61, 90, 91)] == want
        assert g("match_idx", "second_best") == lw["second_best_members"][1] and g("match_idx", "occupied_wins") == lw["occupied_members"][1]
        assert g("reached", "all_claimed") == LR.ABOVE_TH_LOW and g("raw_best_dist", "all_claimed") == 256
        assert g("match_idx", "split_plus_tie", 0) == lw["tie_indices"][0] > lw["tie_indices"][1]
    # the sets are small: K x M in the hundreds
    for inp in sets.values():
        assert len(inp["kfs"]) * len(inp["points" if "points" in inp else "lines"]["max_dist"]) < 1000


def test_the_cut_is_the_references_f32_comparison():
    for th_low in (R.POINT_TH_LOW, R.LINE_TH_LOW):
        for ratio in (0.0, 0.5, 1.0, 1.5, 1.02, 1.0199999, 0.99999994, 2.0, 4.2):
            T = R.cut_of(th_low, ratio)
            lim = np.float32(th_low) * np.float32(ratio)
            assert np.float32(T) <= lim and not np.float32(T + 1) <= lim
    assert R.cut_of(50, 1.0) == 50 and R.cut_of(50, 1.5) == 75 and R.cut_of(60, 1.5) == 90


# ---------------------------------------------------------------------------------------------------------------- the host entries

def test_host_entries_equal_the_golden(sets, golden):
    for sname, inp in sets.items():
        for run, projection, ratio in runs_of(inp):
            out = search(inp, projection, ratio, host=True)
            want = part(golden, sname, run)
            same(out, want, f"{sname} {run} ")
            assert out["stats"].tolist() == [0, windows(want, inp), 0, 0, 0], (sname, run)


SHAPES = [(3, 300, 300, None), (2, 65, 100, 1), (1, 1, 1, None), (5, 257, 40, None)]


@pytest.fixture(scope="module")
def random_sets():
    out = {}
    for K, M, N, empty in SHAPES:
        out[("points", K, M)] = S.random_point_inputs(K, M, N, seed=K + M, empty_kf=empty)
        out[("lines", K, M)] = S.random_line_inputs(K, M, N, seed=K + M, empty_kf=empty)
    return {k: (inp, restate(inp, R.INVZ, 1.5)) for k, inp in out.items()}


@pytest.mark.parametrize("kind", ["points", "lines"])
@pytest.mark.parametrize("shape", SHAPES)
def test_host_entries_equal_the_restatement_at_other_sizes(random_sets, kind, shape):
    inp, want = random_sets[(kind, shape[0], shape[1])]
    same(search(inp, R.INVZ, 1.5, host=True), want)


def test_host_entries_take_the_ambiguous_through_the_hosts_libm():
    for inp in (dict(S.LF.ambiguous_point_inputs(), occupied=None), dict(S.LF.ambiguous_line_inputs(), occupied=None)):
        want = restate(inp, R.CAMERA, 1.5)
        assert want["ambiguous"].sum() >= 12
        same(search(inp, R.CAMERA, 1.5, host=True), want)


def test_one_batched_call_equals_the_sequential_single_calls():
    """The verification loop of src/LoopClosing.cc:1021-1044: one K = 5 call against five K = 1 calls in sequence — key frames are
    independent of each other, each starts from its own `occupied`."""
    from plvs_amd.keyframe import line_loop_search_by_projection_kf, loop_search_by_projection_kf
    pinp, linp = S.repeated_point_inputs(5, 150), S.random_line_inputs(5, 90, 80, seed=12)
    assert (restate(pinp, R.CAMERA, 1.5)["nmatches"] > 20).all(), "the repeated key frame does not see its points under every pose"
    for inp in (pinp, linp):
        points = "points" in inp
        with S.Handles(points_inp=inp if points else None, lines_inp=None if points else inp, host_only=True) as h:
            batch = search(inp, R.CAMERA, 1.5, host=True, handles=h)
            for k in range(5):
                occ = None if inp["occupied"] is None else [inp["occupied"][k]]
                if points:
                    one = loop_search_by_projection_kf([h.kfs[k]], [h.poses[k]], h.points, inp["th"], 1.5, R.CAMERA, inp["skip"][k], occ, host=True)
                else:
                    one = line_loop_search_by_projection_kf([h.kfs[k]], [h.poses[k]], h.lines, inp["th"], 1.5, inp["skip"][k], occ, host=True)
                for key in OUTPUTS:
                    assert (one[key][0] == batch[key][k]).all(), (key, k)


def test_entries_refuse_before_any_device_call(sets):
    from plvs_amd import _lib
    from plvs_amd.keyframe import (_lists, line_loop_search_by_projection_kf, loop_search_by_projection_kf,
                                   loop_search_by_projection_points_and_lines_kf)
    pinp, linp = sets["point"], sets["line"]
    with S.Handles(points_inp=pinp, host_only=True) as P, S.Handles(lines_inp=linp, host_only=True) as Ln:
        def refused(what, f, *a, **kw):
            with pytest.raises(_lib.PlvsHipError) as e:
                f(*a, **kw)
            assert e.value.code == _lib.PLVS_ERR_INVALID_ARG and what in str(e.value), str(e.value)

        for host in (True, False):
            refused("null key-frame handle", loop_search_by_projection_kf, [P.kfs[0], None, P.kfs[2]], P.poses, P.points, host=host)
            refused("null key-frame handle", line_loop_search_by_projection_kf, [None] + Ln.kfs[1:], Ln.poses, Ln.lines, host=host)
            refused("without a line side", line_loop_search_by_projection_kf, P.kfs, P.poses, Ln.lines, host=host)
            refused("without a point side", loop_search_by_projection_kf, Ln.kfs[:3], Ln.poses[:3], P.points, host=host)
            refused("th outside", loop_search_by_projection_kf, P.kfs, P.poses, P.points, th=-1.0, host=host)
            refused("th outside", line_loop_search_by_projection_kf, Ln.kfs, Ln.poses, Ln.lines, th=2.0e6, host=host)
            for ratio in (-0.5, float("nan")):
                refused("ratio_hamming negative or NaN", loop_search_by_projection_kf, P.kfs, P.poses, P.points, ratio_hamming=ratio, host=host)
                refused("ratio_hamming negative or NaN", line_loop_search_by_projection_kf, Ln.kfs, Ln.poses, Ln.lines, ratio_hamming=ratio, host=host)
            refused(">= 256", loop_search_by_projection_kf, P.kfs, P.poses, P.points, ratio_hamming=5.12, host=host)             # 50 * 5.12 = 256
            refused(">= 256", line_loop_search_by_projection_kf, Ln.kfs, Ln.poses, Ln.lines, ratio_hamming=4.2667, host=host)    # 60 * 4.2667 = 256.002
            refused(">= 256", loop_search_by_projection_kf, P.kfs, P.poses, P.points, ratio_hamming=float("inf"), host=host)
            refused("unknown projection", loop_search_by_projection_kf, P.kfs, P.poses, P.points, projection=2, host=host)
            refused("unknown projection", loop_search_by_projection_kf, P.kfs, P.poses, P.points, projection=-1, host=host)
        # the largest ratios that pass: 50 * 5.1 = 255, 60 * 4.25 = 255
        assert loop_search_by_projection_kf(P.kfs, P.poses, P.points, pinp["th"], 5.1, host=True)["nmatches"].sum() > 0
        assert line_loop_search_by_projection_kf(Ln.kfs, Ln.poses, Ln.lines, linp["th"], 4.25, host=True)["nmatches"].sum() > 0
        # a host-only handle in a device entry: refused before any HIP call (this machine may have no device to call)
        refused("PLVS_KEYFRAME_HOST_ONLY", loop_search_by_projection_kf, P.kfs, P.poses, P.points)
        refused("PLVS_KEYFRAME_HOST_ONLY", line_loop_search_by_projection_kf, Ln.kfs, Ln.poses, Ln.lines)
        refused("PLVS_KEYFRAME_HOST_ONLY", loop_search_by_projection_points_and_lines_kf, P.kfs, P.poses, points=P.points)
        refused("neither points nor lines", loop_search_by_projection_points_and_lines_kf, P.kfs, P.poses)
        refused(">= 256", loop_search_by_projection_points_and_lines_kf, P.kfs, P.poses, points=P.points, ratio_hamming_points=6.0)
        # nothing written by a refused call: through the C entries, sentinel fills
        vp, fl = ctypes.c_void_p, ctypes.c_float
        K, hs, ps = _lists(P.kfs, P.poses)
        pc = P.points.as_c()
        for name, tail in (("plvs_hip_orb_loop_search_by_projection_kf", [None]), ("plvs_hip_orb_loop_search_by_projection_kf_host", [])):
            f = getattr(_lib.lib, name)
            f.argtypes = [vp, vp, ctypes.c_int, vp, vp, vp, fl, fl, ctypes.c_int, vp, vp, vp, vp, vp] + [vp] * len(tail)
            for poses, th, ratio, proj, what in ((None, 4.0, 1.5, 0, "null poses"), (ps, -1.0, 1.5, 0, "th outside"), (ps, 4.0, -1.0, 0, "ratio_hamming"),
                                                 (ps, 4.0, 5.12, 0, ">= 256"), (ps, 4.0, 1.5, 7, "unknown projection")):
                idx, dist = np.full((K, pc.m), -7, np.int32), np.full((K, pc.m), -7, np.int32)
                rch, nm, st = np.full((K, pc.m), 77, np.uint8), np.full(K, -7, np.int32), np.full(5, -1, np.int32)
                rc = f(hs, poses, K, ctypes.byref(pc), None, None, th, ratio, proj, _lib.np_ptr(idx), _lib.np_ptr(dist), _lib.np_ptr(rch), _lib.np_ptr(nm),
                       _lib.np_ptr(st), *tail)
                assert rc == _lib.PLVS_ERR_INVALID_ARG and what in _lib.lib.plvs_hip_last_error().decode(), what
                assert (idx == -7).all() and (dist == -7).all() and (rch == 77).all() and (nm == -7).all() and st.tolist() == [-1] * 5, what


def test_the_wide_theta_interval_refuses_the_line_call_and_writes_nothing(sets):
    from plvs_amd import _lib
    kfs = [dict(kf) for kf in sets["line"]["kfs"]]
    kfs[1]["scale_factors"] = np.array([1.0, 10.0, 1.44], np.float32)      # deltaTheta = 100 degrees at level 1
    inp = dict(sets["line"], kfs=kfs)
    with pytest.raises(_lib.PlvsHipError) as e:
        search(inp, None, 1.5, host=True)
    assert e.value.code == _lib.PLVS_ERR_INVALID_ARG and "theta" in str(e.value)
    # key frame 0's pairs were decided before the wide pair was met: still nothing is written
    vp, fl = ctypes.c_void_p, ctypes.c_float
    from plvs_amd.keyframe import _lists
    with S.Handles(lines_inp=inp, host_only=True) as h:
        K, hs, ps = _lists(h.kfs, h.poses)
        lc = h.lines.as_c()
        f = _lib.lib.plvs_hip_line_loop_search_by_projection_kf_host
        f.argtypes = [vp, vp, ctypes.c_int, vp, vp, vp, fl, fl, vp, vp, vp, vp, vp]
        idx, dist, nm = np.full((K, lc.m), -7, np.int32), np.full((K, lc.m), -7, np.int32), np.full(K, -7, np.int32)
        rc = f(hs, ps, K, ctypes.byref(lc), _lib.np_ptr(np.ascontiguousarray(inp["skip"])), None, inp["th"], 1.5, _lib.np_ptr(idx), _lib.np_ptr(dist), None,
               _lib.np_ptr(nm), None)
        assert rc == _lib.PLVS_ERR_INVALID_ARG and (idx == -7).all() and (dist == -7).all() and (nm == -7).all()


def test_header_declares_and_library_exports_the_loop_search_entries():
    from plvs_amd import _lib, keyframe
    with open(os.path.join(ROOT, "include", "plvs_hip.h")) as fh:
        header = fh.read()
    for name in ENTRIES:
        assert re.search(r"\bint " + name + r"\(\s*const plvs_keyframe\* const\* kfs, const plvs_keyframe_sim3_pose\* sim3_poses, int n_kfs", header), name
        assert hasattr(_lib.lib, name), name
    assert re.search(r"#define PLVS_LOOP_PROJECT_CAMERA 0\b", header) and re.search(r"#define PLVS_LOOP_PROJECT_INVZ 1\b", header)
    assert (keyframe.PROJECT_CAMERA, keyframe.PROJECT_INVZ) == (0, 1) == (R.CAMERA, R.INVZ)
    assert _lib.lib.plvs_hip_abi_version() == 1
    with open(os.path.join(ROOT, "include", "plvs_hip.hpp")) as fh:
        hpp = fh.read()
    assert hpp.count("inline int LoopSearchByProjection(") == 2 and "inline int LoopSearchByProjectionPointsAndLines(" in hpp
    for name in ("loop_search_by_projection_kf", "line_loop_search_by_projection_kf", "loop_search_by_projection_points_and_lines_kf"):
        assert callable(getattr(keyframe, name)), name
    with open(os.path.join(ROOT, "plvs_amd", "csrc", "loop_search_pair.hpp")) as fh:
        assert re.search(r"constexpr int kListLen = (\d+);", fh.read()).group(1) == str(L)


# ---------------------------------------------------------------------------------------------------------------- the pair headers alone

FLAGS = ["-std=c++14", "-ffp-contract=off", "-Wall", "-Wextra", "-Werror"]
PAIR_SRC = os.path.join(ROOT, "tests", "host", "loop_search_pair_host.cpp")


def _write_extra(path, inp, projection, ratio):
    with open(path, "wb") as f:
        f.write(struct.pack("<fi", ratio, 0 if projection is None else projection))
        for k in range(len(inp["kfs"])):
            o = None if inp["occupied"] is None else inp["occupied"][k]
            f.write(struct.pack("<i", -1 if o is None else len(o)) + (b"" if o is None else np.ascontiguousarray(o, np.uint8).tobytes()))


def _check_pair_program(exe, sets, golden, tmp_path, env=None):
    from tests.test_line_fuse import _write_pair_input as write_lines
    from tests.test_orb_fuse import _write_pair_input as write_points
    errors, truncated = "", 0
    for sname, inp in sets.items():
        kind = "points" if "points" in inp else "lines"
        path, extra = str(tmp_path / (sname + "_input.bin")), str(tmp_path / (sname + "_extra.bin"))
        (write_points if kind == "points" else write_lines)(path, inp)
        for run, projection, ratio in runs_of(inp):
            _write_extra(extra, inp, projection, ratio)
            for mode in ((kind, "lists") if kind == "points" else (kind,)):
                r = subprocess.run([exe, mode, path, extra], capture_output=True, text=True, env=env)
                assert r.returncode == 0 and "loop_search_pair ok" in r.stdout, r.stderr + r.stdout[-500:]
                got = np.array([[int(c) for c in ln.split()[1:]] for ln in r.stdout.splitlines() if ln.startswith("pair ")], np.int64)
                want = np.stack([golden[f"{sname}_{run}_{k}"].reshape(-1).astype(np.int64) for k in OUTPUTS[:3]], 1)
                assert got.shape == want.shape and (got == want).all(), (sname, run, mode, np.argwhere(got != want)[:8])
                said = np.array([[int(c) for c in ln.split()[1:]] for ln in r.stdout.splitlines() if ln.startswith("nmatches ")], np.int64)
                assert (said[:, 1] == golden[f"{sname}_{run}_nmatches"]).all(), (sname, run, mode)
                if mode == "lists" and sname == "point_crowd":
                    truncated += int(said[:, 2].sum())
                errors += r.stderr
    assert truncated >= 2 * 2, "the crowd's truncated, wholly claimed lists were not recomputed"
    return errors


@pytest.mark.parametrize("compiler", ["g++", "/opt/rocm/llvm/bin/clang++"])
def test_pair_headers_alone_reproduce_the_reference(sets, golden, tmp_path, compiler):
    """loop_search_pair.hpp with fuse_pair.hpp and line_fuse_pair.hpp — the text the kernels and the entries compile — as a stand-alone
    host program under g++ and ROCm's clang: the host twins' path, and for points the device entry's path over lists built serially."""
    if not os.path.exists(compiler) and compiler != "g++":
        pytest.fail(f"{compiler} is missing")
    exe = str(tmp_path / "loop_search_pair_host")
    subprocess.run([compiler, "-O2"] + FLAGS + [PAIR_SRC, "-o", exe], check=True)
    _check_pair_program(exe, sets, golden, tmp_path)


def test_pair_headers_under_the_sanitizers(sets, golden, tmp_path):
    exe = str(tmp_path / "loop_search_pair_host_san")
    subprocess.run(["g++", "-O1", "-g"] + FLAGS + ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", PAIR_SRC, "-o", exe], check=True)
    err = _check_pair_program(exe, sets, golden, tmp_path, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1"))
    assert "ERROR: AddressSanitizer" not in err and "runtime error" not in err, err


# ---------------------------------------------------------------------------------------------------------------- GPU

@pytest.mark.gpu
def test_device_golden_scenario_and_crowd_with_both_projections(sets, golden):
    for sname, inp in sets.items():
        for run, projection, ratio in runs_of(inp):
            out = search(inp, projection, ratio, host=False)
            want = part(golden, sname, run)
            same(out, want, f"{sname} {run} ")
            assert out["stats"][1:3].tolist() == [windows(want, inp), 1] and out["stats"][3] > 0, (sname, run)


@pytest.mark.gpu
def test_device_stats_count_the_recomputed_lists(sets):
    for sname in ("point_crowd", "line_crowd"):
        inp = sets[sname]
        out = search(inp, R.CAMERA, 1.5, host=False)
        assert out["stats"][4] >= 1, sname                   # the last of the L + 2 same-descriptor items (a line's theta may hand one to the host whole: stats[0])
        assert out["stats"][0] + out["stats"][4] >= 2, sname
        host = search(inp, R.CAMERA, 1.5, host=True)
        same(out, host)
    # windows of fewer than L members at or below the cut: nothing is recomputed
    for inp in (S.random_point_inputs(3, 300, 60, seed=8), S.random_line_inputs(3, 120, 12, seed=8)):
        c = {}
        if "points" in inp:
            want = R.point_search(inp["kfs"], inp["points"], inp["skip"], inp["occupied"], inp["th"], 1.5, R.CAMERA, c)
        else:
            want = R.line_search(inp["kfs"], inp["lines"], inp["skip"], inp["occupied"], inp["th"], 1.5, c)
        assert c["windows_over_list_len"] == 0 and want["nmatches"].sum() > 0
        out = search(inp, R.CAMERA, 1.5, host=False)
        same(out, want)
        assert out["stats"][4] == 0


@pytest.mark.gpu
def test_device_combined_entry_equals_the_two_single_entries(sets):
    from plvs_amd.keyframe import (line_loop_search_by_projection_kf, loop_search_by_projection_kf,
                                   loop_search_by_projection_points_and_lines_kf)
    pinp, linp = S.random_point_inputs(3, 140, 120, seed=41), S.random_line_inputs(3, 90, 80, seed=41)
    with S.Handles(points_inp=pinp, lines_inp=linp) as h:
        p1 = loop_search_by_projection_kf(h.kfs, h.poses, h.points, 8.0, 1.5, R.INVZ, pinp["skip"], pinp["occupied"])
        l1 = line_loop_search_by_projection_kf(h.kfs, h.poses, h.lines, 3.0, 1.0, linp["skip"], linp["occupied"])
        p2, l2, stats = loop_search_by_projection_points_and_lines_kf(h.kfs, h.poses, h.points, 8.0, 1.5, R.INVZ, pinp["skip"], pinp["occupied"],
                                                                      h.lines, 3.0, 1.0, linp["skip"], linp["occupied"])
        same(p2, p1, "points ")
        same(l2, l1, "lines ")
        assert p2["stats"].tolist() == p1["stats"].tolist() and l2["stats"].tolist() == l1["stats"].tolist()
        assert stats.tolist() == [2, 1, int(p1["stats"][3] + l1["stats"][3])]          # two launches, ONE wait
        none, l3, stats = loop_search_by_projection_points_and_lines_kf(h.kfs, h.poses, lines=h.lines, th_lines=3.0, ratio_hamming_lines=1.0,
                                                                        skip_lines=linp["skip"], occupied_lines=linp["occupied"])
        assert none is None and stats.tolist() == [1, 1, int(l1["stats"][3])]
        same(l3, l1)
    # the line poses of the shared handles are the line set's own: the line results are the restatement's
    same(l1, R.line_search(linp["kfs"], linp["lines"], linp["skip"], linp["occupied"], 3.0, 1.0))


@pytest.mark.gpu
@pytest.mark.parametrize("K", [1, 2, 5])
@pytest.mark.parametrize("M", [0, 1, 255, 256, 257, 513])
def test_device_sieve_tile_edges_against_the_host_twin(K, M):
    from plvs_amd.orbmatcher import FusePoints
    inp = S.random_point_inputs(K, max(M, 1), 80, seed=100 * K + M)
    with S.Handles(points_inp=inp) as h:
        if M == 0:
            z3, z1, zd = np.zeros((0, 3), np.float32), np.zeros(0, np.float32), np.zeros((0, 32), np.uint8)
            h.points = FusePoints(z3, z3, z1, z1, zd)
            inp = dict(inp, skip=None)
        for projection in (R.CAMERA, R.INVZ):
            out = search(inp, projection, 1.5, host=False, handles=h)
            same(out, search(inp, projection, 1.5, host=True, handles=h), f"projection {projection} ")
            launched = M > 0 and not (inp["skip"] != 0).all()
            assert out["match_idx"].shape == (K, M) and out["stats"][2] == int(launched)
    ln = S.random_line_inputs(K, max(M, 1) if M < 300 else 130, 40, seed=100 * K + M)
    with S.Handles(lines_inp=ln) as h:
        same(search(ln, None, 1.5, host=False, handles=h), search(ln, None, 1.5, host=True, handles=h), "lines ")


@pytest.mark.gpu
def test_device_key_frames_without_features():
    for inp in (S.random_point_inputs(3, 130, 60, seed=21, empty_kf=1), S.random_line_inputs(3, 70, 60, seed=21, empty_kf=0)):
        want = restate(inp, R.CAMERA, 1.5)
        out = search(inp, R.CAMERA, 1.5, host=False)
        same(out, want)
        assert out["stats"][2] == 1


@pytest.mark.gpu
def test_device_occupied_with_one_null_entry_among_the_others():
    for inp in (S.random_point_inputs(3, 200, 150, seed=5, occupied_fraction=0.5), S.random_line_inputs(3, 100, 90, seed=5, occupied_fraction=0.5)):
        assert inp["occupied"][1] is None and inp["occupied"][0].any() and inp["occupied"][2].any()
        want = restate(inp, R.INVZ, 1.5)
        out = search(inp, R.INVZ, 1.5, host=False)
        same(out, want)
        free = restate(dict(inp, occupied=None), R.INVZ, 1.5)
        assert (free["match_idx"][0] != want["match_idx"][0]).any(), "occupied changes nothing"
        assert (free["match_idx"][1] == want["match_idx"][1]).all()
        for k in (0, 2):       # nothing occupied on entry is ever matched
            m = want["match_idx"][k]
            assert not inp["occupied"][k][m[m >= 0]].any()


@pytest.mark.gpu
def test_device_launch_free_shapes():
    from plvs_amd.keyframe import line_loop_search_by_projection_kf, loop_search_by_projection_kf
    pinp, linp = S.random_point_inputs(2, 40, 50, seed=31), S.random_line_inputs(2, 40, 50, seed=31)
    for inp in (pinp, linp):
        out = search(dict(inp, skip=np.ones_like(inp["skip"])), R.CAMERA, 1.5, host=False)
        assert out["stats"].tolist() == [0] * 5 and (out["reached"] == 0).all() and (out["match_idx"] == -1).all() and (out["nmatches"] == 0).all()
        empty = dict(inp, occupied=None,
                     kfs=[dict(kf, **({"x": kf["x"][:0], "y": kf["y"][:0], "octave": kf["octave"][:0], "u_right": kf["u_right"][:0],
                                       "desc": kf["desc"][:0]} if "points" in inp else
                                      {"kl": kf["kl"][:0], "desc": kf["desc"][:0], "u_right_start": None, "u_right_end": None}))
                          for kf in inp["kfs"]])
        out = search(empty, R.CAMERA, 1.5, host=False)
        same(out, restate(empty, R.CAMERA, 1.5))
        assert out["stats"][2:].tolist() == [0, 0, 0]
    with S.Handles(points_inp=pinp, lines_inp=linp) as h:
        out = loop_search_by_projection_kf([], [], h.points)
        assert out["match_idx"].shape == (0, 40) and out["stats"].tolist() == [0] * 5
        out = line_loop_search_by_projection_kf([], [], h.lines)
        assert out["match_idx"].shape == (0, 40) and out["stats"].tolist() == [0] * 5


@pytest.mark.gpu
def test_device_ambiguous_pairs_come_back_as_the_hosts():
    for inp in (dict(S.LF.ambiguous_point_inputs(), occupied=None), dict(S.LF.ambiguous_line_inputs(), occupied=None)):
        want = restate(inp, R.CAMERA, 1.5)
        out = search(inp, R.CAMERA, 1.5, host=False)
        same(out, search(inp, R.CAMERA, 1.5, host=True))
        same(out, want)
        assert 12 <= out["stats"][0] <= int(want["ambiguous"].sum())


@pytest.mark.gpu
def test_device_refusals_launch_nothing_and_write_nothing(sets):
    from plvs_amd import _lib
    from plvs_amd.keyframe import _lists
    pinp = sets["point"]
    vp, fl = ctypes.c_void_p, ctypes.c_float
    with S.Handles(points_inp=pinp) as P:
        K, hs, ps = _lists(P.kfs, P.poses)
        bad = (vp * K)(*[None if k == 1 else P.kfs[k].handle for k in range(K)])
        pc = P.points.as_c()
        f = _lib.lib.plvs_hip_orb_loop_search_by_projection_kf
        f.argtypes = [vp, vp, ctypes.c_int, vp, vp, vp, fl, fl, ctypes.c_int, vp, vp, vp, vp, vp, vp]
        for handles, poses, th, ratio, proj, idx_null in ((bad, ps, 4.0, 1.5, 0, False), (hs, None, 4.0, 1.5, 0, False), (hs, ps, -1.0, 1.5, 0, False),
                                                          (hs, ps, 4.0, 1.5, 0, True), (hs, ps, 4.0, float("nan"), 0, False), (hs, ps, 4.0, 5.12, 1, False),
                                                          (hs, ps, 4.0, 1.5, 2, False)):
            idx, dist = np.full((K, pc.m), -7, np.int32), np.full((K, pc.m), -7, np.int32)
            nm, st = np.full(K, -7, np.int32), np.full(5, -1, np.int32)
            rc = f(handles, poses, K, ctypes.byref(pc), None, None, th, ratio, proj, None if idx_null else _lib.np_ptr(idx), _lib.np_ptr(dist), None,
                   _lib.np_ptr(nm), _lib.np_ptr(st), None)
            assert rc == _lib.PLVS_ERR_INVALID_ARG and (idx == -7).all() and (dist == -7).all() and (nm == -7).all() and st.tolist() == [-1] * 5


@pytest.mark.gpu
def test_device_the_same_handle_twice_with_two_poses(sets):
    from plvs_amd.keyframe import loop_search_by_projection_kf
    inp = sets["point"]
    two = dict(inp, kfs=[inp["kfs"][0], dict(inp["kfs"][0], **{k: inp["kfs"][1][k] for k in ("q_cw", "Rcw", "tcw", "Ow_points", "Ow_lines")})],
               skip=None, occupied=[inp["occupied"][0], None])
    want = restate(two, R.CAMERA, 1.5)
    with S.Handles(points_inp=inp) as h:
        out = loop_search_by_projection_kf([h.kfs[0], h.kfs[0]], [h.poses[0], h.poses[1]], h.points, inp["th"], 1.5, R.CAMERA, None, two["occupied"])
    same(out, want)
    assert (want["reached"][0] != want["reached"][1]).any()


@pytest.mark.gpu
def test_device_one_batched_call_equals_five_single_calls():
    from plvs_amd.keyframe import loop_search_by_projection_kf
    inp = S.repeated_point_inputs(5, 300)
    with S.Handles(points_inp=inp) as h:
        batch = search(inp, R.CAMERA, 1.5, host=False, handles=h)
        for k in range(5):
            one = loop_search_by_projection_kf([h.kfs[k]], [h.poses[k]], h.points, inp["th"], 1.5, R.CAMERA, inp["skip"][k])
            for key in OUTPUTS:
                assert (one[key][0] == batch[key][k]).all(), (key, k)
    same(batch, restate(inp, R.CAMERA, 1.5))
