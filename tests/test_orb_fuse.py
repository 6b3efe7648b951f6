"""The search stage of ORBmatcher::Fuse for K key frames x M points in one call (plvs_hip_orb_fuse_search, its host twin
plvs_hip_orb_fuse_search_host, plvs_amd/csrc/fuse_pair.hpp) against the reference's own compiled definitions
(tests/golden/orb_fuse_reference.npz, scripts/make_orb_fuse_golden.py), and the replay rule of INTEGRATION.md on a toy map
(tests/orb_fuse_replay.py).  Every index, distance and stage is compared for equality."""
import dataclasses
import json
import os
import re
import struct
import subprocess

import numpy as np
import pytest

from tests import orb_fuse_replay as P
from tests import orb_fuse_restatement as R
from tests import orb_fuse_scenario as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "orb_fuse_reference.npz")
FACTS = os.path.join(ROOT, "tests", "golden", "orb_fuse_reference_facts.json")
OUTPUTS = ("best_idx", "best_dist", "reached")


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
def restated(scenario, crowd):
    return (R.fuse_search(scenario["kfs"], scenario["points"], scenario["skip"], scenario["th"]),
            R.fuse_search(crowd["kfs"], crowd["points"], None, crowd["th"]))


def _search(inp, host, skip="own", **kw):
    from plvs_amd.orbmatcher import ORBmatcher
    kfs, pts = S.views(inp)
    return ORBmatcher().FuseSearch(kfs, pts, inp["th"], inp["skip"] if isinstance(skip, str) else skip, host=host, **kw)


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
        for k in ("reached", "raw_best_dist", "n_dist", "u", "v", "best_idx", "best_dist"):
            a, b = r[k], golden[pre + k]
            assert a.dtype == b.dtype and a.tobytes() == b.tobytes(), pre + k
        # bestIdx is observable in the reference where bestDist <= TH_LOW only (GetMapPoint(bestIdx))
        assert (golden[pre + "raw_best_idx"] == r["best_idx"]).all()


def test_golden_run_takes_every_stage_and_every_placed_case(scenario, golden, facts):
    counts, w = facts["facts"]["counts"], scenario["where"]
    for code, name in enumerate(R.REACHED):
        assert counts[name] >= 1 and int((golden["reached"] == code).sum()) == counts[name], name
    for name in ("dropped_below_level", "dropped_above_level", "dropped_mono_gate", "dropped_stereo_gate", "u_right_zero_stereo_branch",
                 "clipped_left", "clipped_right", "clipped_top", "clipped_bottom", "tie_winner_not_lowest_index"):
        assert counts[name] >= 1, name
    assert facts["facts"]["log_overload"] == "std::log(float)" and facts["facts"]["double_overload"] == 0
    at = lambda name, k=0: int(golden["reached"][k, w[name][0]])
    # the placed windows hold ONE key point each: which gate dropped it is the case's own
    assert [at(n) for n in ("below_level", "above_level", "mono_gate", "stereo_gate", "u_right_zero")] == [R.NO_CANDIDATE] * 5
    assert [int(golden["n_dist"][0, w[n][0]]) for n in ("below_level", "above_level", "mono_gate", "stereo_gate", "u_right_zero")] == [0] * 5
    i = w["u_right_zero"][0]
    kf0 = scenario["kfs"][0]
    assert (kf0["u_right"] == 0).sum() == 1                         # mvuRight == 0.0f takes the stereo branch: with `> 0` the mono
    fr = R.front(kf0, scenario["points"])                           # gate would have accepted it (ex, ey far inside 5.99)
    j = int(np.flatnonzero(kf0["u_right"] == 0)[0])
    e2 = (fr["u"][i] - kf0["x"][j]) ** 2 + (fr["v"][i] - kf0["y"][j]) ** 2
    assert float(e2) * float(kf0["inv_level_sigma2"][kf0["octave"][j]]) < 1.0
    for n in ("clip_left", "clip_right", "clip_top", "clip_bottom", "candidate_mono", "candidate_stereo", "candidate_level_minus_1", "tie"):
        assert at(n) == R.CANDIDATE, n
    ja, jb = w["tie_indices"]
    assert ja > jb and int(golden["raw_best_idx"][0, w["tie"][0]]) == ja
    assert at("above_th_low") == R.ABOVE_TH_LOW and int(golden["raw_best_dist"][0, w["above_th_low"][0]]) > 50
    assert at("z_zero_nan", 2) == R.OUTSIDE and np.isnan(golden["u"][2, w["z_zero_nan"][0]])
    assert at("z_zero_inf", 2) == R.OUTSIDE and np.isinf(golden["u"][2, w["z_zero_inf"][0]])
    assert facts["facts"]["crowd_counts"]["tie_winner_not_lowest_index"] >= 1


def test_host_entry_equals_the_golden(scenario, crowd, golden):
    out = _search(scenario, host=True)
    _same(out, golden)
    assert out["stats"].tolist() == [0, _window_pairs(golden), 0]
    _same(_search(crowd, host=True), {k: golden["crowd_" + k] for k in OUTPUTS}, what="crowd ")


@pytest.mark.parametrize("shape", [(3, 300, 300, None), (2, 65, 100, 1), (1, 1, 1, None), (3, 63, 40, 0)])
def test_host_entry_equals_the_restatement_at_other_sizes(shape):
    K, M, N, empty = shape
    inp = S.random_inputs(K, M, N, seed=K + M, empty_kf=empty)
    _same(_search(inp, host=True), R.fuse_search(inp["kfs"], inp["points"], inp["skip"], inp["th"]))


def test_host_entry_takes_the_ambiguous_levels_through_the_hosts_logarithm():
    inp = S.ambiguous_inputs()
    c = {}
    want = R.fuse_search(inp["kfs"], inp["points"], inp["skip"], inp["th"], c)
    assert c["ambiguous"] >= 1
    _same(_search(inp, host=True), want)


def test_zero_distance_is_reported_at_the_viewing_angle(scenario):
    """dist3D == 0 gives a ratio of infinity and no defined level in the reference; no consistent pose reaches it (the camera centre
    projects nowhere), so the reference's run has none.  With GetCameraCenter() handed in equal to a visible point the entries report
    the pair as rejected at the viewing angle, as the local-map link does."""
    i = scenario["where"]["candidate_mono"][0]
    kf = dict(scenario["kfs"][0], Ow=scenario["points"]["pos"][i].copy())
    pts = {k: v.copy() for k, v in scenario["points"].items()}
    pts["min_dist"][i] = 0                      # (or the band's lower edge rejects the pair first)
    inp = dict(kfs=[kf], points=pts, skip=None, th=scenario["th"])
    c = {}
    want = R.fuse_search(inp["kfs"], inp["points"], None, inp["th"], c)
    assert c["dist3d_zero"] == 1 and want["reached"][0, i] == R.VIEW_ANGLE
    _same(_search(inp, host=True), want)


def test_host_entry_refuses_what_the_device_entry_refuses(scenario):
    from plvs_amd import _lib
    from plvs_amd.orbmatcher import ORBmatcher
    kfs, pts = S.views(scenario)
    for change in (dict(n_cameras=2), dict(camera_model=1)):
        bad = [kfs[0], dataclasses.replace(kfs[1], **change), kfs[2]]
        with pytest.raises(_lib.PlvsHipError) as e:
            ORBmatcher().FuseSearch(bad, pts, 3.0, scenario["skip"], host=True)
        assert e.value.code == _lib.PLVS_ERR_INVALID_ARG
    with pytest.raises(_lib.PlvsHipError) as e:
        ORBmatcher().FuseSearch(kfs, pts, 3.0, scenario["skip"], host=True, outputs=False)
    assert e.value.code == _lib.PLVS_ERR_INVALID_ARG


def _write_pair_input(path, inp):
    K, M = len(inp["kfs"]), len(inp["points"]["min_dist"])
    with open(path, "wb") as f:
        f.write(struct.pack("<iif", K, M, inp["th"]))
        for kf in inp["kfs"]:
            f32 = lambda a: np.ascontiguousarray(a, np.float32).tobytes()
            f.write(f32(kf["q_cw"]) + f32(kf["tcw"]) + f32(kf["Ow"]) + f32(kf["K4"]) + f32([kf["mbf"]]) + f32(kf["bounds4"]) +
                    f32([kf["min_x"], kf["min_y"], kf["grid_w_inv"], kf["grid_h_inv"], kf["log_scale_factor"]]))
            f.write(struct.pack("<ii", len(kf["scale_factors"]), len(kf["x"])))
            f.write(f32(kf["x"]) + f32(kf["y"]) + np.ascontiguousarray(kf["octave"], np.int32).tobytes() + f32(kf["u_right"]) +
                    np.ascontiguousarray(kf["desc"], np.uint8).tobytes() + f32(kf["scale_factors"]) + f32(kf["inv_level_sigma2"]))
        p = inp["points"]
        f.write(b"".join(np.ascontiguousarray(p[k], np.float32).tobytes() for k in ("pos", "normal", "min_dist", "max_dist")))
        f.write(np.ascontiguousarray(p["desc"], np.uint8).tobytes())
        f.write(np.ascontiguousarray(inp["skip"] if inp["skip"] is not None else np.zeros((K, M)), np.uint8).tobytes())


def _check_pair_program(exe, inp, golden, tmp_path, env=None):
    path = str(tmp_path / "fuse_pair_input.bin")
    _write_pair_input(path, inp)
    r = subprocess.run([exe, path], capture_output=True, text=True, env=env)
    assert r.returncode == 0 and "fuse_pair ok" in r.stdout, r.stderr + r.stdout[-500:]
    got = np.array([[int(c) for c in ln.split()[1:]] for ln in r.stdout.splitlines() if ln.startswith("pair ")], np.int64)
    want = np.stack([golden[k].reshape(-1).astype(np.int64) for k in OUTPUTS], 1)
    assert got.shape == want.shape and (got == want).all(), np.argwhere(got != want)[:8]
    return r


FLAGS = ["-std=c++14", "-ffp-contract=off", "-Wall", "-Wextra", "-Werror"]
HOST_SRC = os.path.join(ROOT, "tests", "host", "fuse_pair_host.cpp")


@pytest.mark.parametrize("compiler", ["g++", "/opt/rocm/llvm/bin/clang++"])
def test_pair_header_on_the_host_reproduces_the_reference(scenario, golden, tmp_path, compiler):
    """plvs_amd/csrc/fuse_pair.hpp — the text the kernel compiles — as a stand-alone host program under g++ and ROCm's clang."""
    if not os.path.exists(compiler) and compiler != "g++":
        pytest.fail(f"{compiler} is missing")
    exe = str(tmp_path / "fuse_pair_host")
    subprocess.run([compiler, "-O2"] + FLAGS + [HOST_SRC, "-o", exe], check=True)
    _check_pair_program(exe, scenario, golden, tmp_path)


def test_pair_header_under_the_sanitizers(scenario, golden, tmp_path):
    exe = str(tmp_path / "fuse_pair_host_san")
    subprocess.run(["g++", "-O1", "-g"] + FLAGS + ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", HOST_SRC, "-o", exe], check=True)
    r = _check_pair_program(exe, scenario, golden, tmp_path, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1"))
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr


def test_header_declares_and_library_exports_both_entries():
    from plvs_amd import _lib
    with open(os.path.join(ROOT, "include", "plvs_hip.h")) as fh:
        header = fh.read()
    for name in ("plvs_hip_orb_fuse_search", "plvs_hip_orb_fuse_search_host"):
        assert re.search(r"\bint " + name + r"\(const plvs_fuse_keyframe\* kfs, int n_kfs, const plvs_fuse_points\* P", header), name
        assert hasattr(_lib.lib, name), name
    assert "typedef struct plvs_fuse_keyframe" in header and "typedef struct plvs_fuse_points" in header
    assert _lib.lib.plvs_hip_abi_version() == 1
    with open(os.path.join(ROOT, "include", "plvs_hip.hpp")) as fh:
        assert "FuseSearch" in fh.read()


def _searcher(host):
    def search(kfs, pts, skip):
        return _search(dict(kfs=kfs, points=pts, skip=skip, th=S.TH), host=host, skip=skip)["best_idx"]
    return search


def _check_replay(batch_host):
    inp = P.replay_inputs()
    host = _searcher(True)
    want = P.sequential(inp, host)
    log = []
    got = P.replayed(inp, host, batch_search=_searcher(batch_host), log=log)
    assert got.state() == want.state()
    M = inp["M"]
    assert any(loser < M for loser, _ in want.replacements), "no current point was replaced by an older one"
    assert any(loser >= M for loser, _ in want.replacements), "no older point was replaced by a current one"
    assert any(stale != live for _, _, stale, live in log), "no dirty point whose stale candidate differs from its live one"
    # and the rule is needed: the batch's candidates with the live re-tests but without the re-query of dirty points end elsewhere
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
def test_device_chained_layout_equals_the_fused_one(scenario, golden):
    from plvs_amd.orbmatcher import fuse_test_chained
    fuse_test_chained(True)
    try:
        out = _search(scenario, host=False)
    finally:
        fuse_test_chained(False)
    _same(out, golden)
    assert out["stats"][2] == 2


@pytest.mark.gpu
@pytest.mark.parametrize("n_kfs", [1, 3])
@pytest.mark.parametrize("m", [1, 63, 64, 65, 257])
def test_device_block_edge_sizes(m, n_kfs):
    inp = S.random_inputs(n_kfs, m, 120, seed=m, empty_kf=1 if n_kfs == 3 else None)
    want = R.fuse_search(inp["kfs"], inp["points"], inp["skip"], inp["th"])
    out = _search(inp, host=False)
    _same(out, want)
    assert out["stats"][1] == _window_pairs(want) and out["stats"][2] == 1


@pytest.mark.gpu
def test_device_crowd_turns_the_stride_loop(crowd, golden):
    g = R.grid_of(crowd["kfs"][0])
    assert int(np.diff(g[0]).reshape(R.GRID_COLS, R.GRID_ROWS).sum(1).max()) > 128      # one column holds more than two strides
    want = {k: golden["crowd_" + k] for k in OUTPUTS}
    kf = crowd["kfs"][0]
    order = g[1]
    for i in range(len(want["best_idx"][0])):                                          # equal distances on both sides of a stride boundary
        d = R._POP[kf["desc"][order] ^ crowd["points"]["desc"][i][None, :]].sum(1)
        tied = np.flatnonzero(d == want["best_dist"][0, i])
        if len(tied) and tied.min() < 64 <= tied.max():
            break
    else:
        pytest.fail("no tie across a stride boundary in the crowd")
    _same(_search(crowd, host=False), want)


@pytest.mark.gpu
def test_device_ambiguous_levels_go_through_the_host():
    inp = S.ambiguous_inputs()
    out, host = _search(inp, host=False), _search(inp, host=True)
    assert out["stats"][0] >= 1
    _same(out, host)
    _same(out, R.fuse_search(inp["kfs"], inp["points"], inp["skip"], inp["th"]))


@pytest.mark.gpu
def test_device_refusals_launch_nothing(scenario):
    from plvs_amd import _lib
    from plvs_amd.orbmatcher import ORBmatcher
    kfs, pts = S.views(scenario)
    for change in (dict(n_cameras=2), dict(camera_model=1)):
        bad = [kfs[0], dataclasses.replace(kfs[1], **change), kfs[2]]
        with pytest.raises(_lib.PlvsHipError) as e:
            ORBmatcher().FuseSearch(bad, pts, 3.0, scenario["skip"])
        assert e.value.code == _lib.PLVS_ERR_INVALID_ARG
    with pytest.raises(_lib.PlvsHipError) as e:
        ORBmatcher().FuseSearch(kfs, pts, 3.0, scenario["skip"], outputs=False)
    assert e.value.code == _lib.PLVS_ERR_INVALID_ARG


@pytest.mark.gpu
@pytest.mark.parametrize("shape", ["no_kfs", "no_points", "empty_kf", "all_skipped"])
def test_device_empty_shapes_launch_nothing(shape):
    inp = S.random_inputs(0 if shape == "no_kfs" else 2, 0 if shape == "no_points" else 40, 60, seed=4)
    if shape == "empty_kf":
        inp = S.random_inputs(1, 40, 60, seed=4, empty_kf=0)
    if shape == "all_skipped":
        inp["skip"] = np.ones_like(inp["skip"])
    out = _search(inp, host=False)
    assert out["stats"][2] == 0 and out["stats"][0] == 0
    if shape in ("empty_kf", "all_skipped"):
        want = R.fuse_search(inp["kfs"], inp["points"], inp["skip"], inp["th"])
        _same(out, want)
        assert (out["reached"] == R.SKIPPED).all() if shape == "all_skipped" else (out["reached"] <= R.EMPTY_WINDOW).all()
    else:
        assert out["best_idx"].size == 0


@pytest.mark.gpu
def test_device_replay_equals_the_sequential_loop():
    _check_replay(batch_host=False)
