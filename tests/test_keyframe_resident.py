"""Key frames resident in a handle (plvs_hip_keyframe_create) and the Fuse searches over handles, on the host: host-only handles and
the _kf_host entries against the compiled reference's recorded run (tests/golden/orb_fuse_reference.npz, line_fuse_reference.npz) and
against the non-resident _host entries, which are pinned to those goldens (tests/test_orb_fuse.py, tests/test_line_fuse.py).  The
device entries are in tests/test_keyframe_resident_gpu.py."""
import ctypes
import dataclasses
import os
import re
import subprocess

import numpy as np
import pytest

from tests import keyframe_resident_util as U
from tests import line_fuse_restatement as LR
from tests import line_fuse_scenario as LS
from tests import orb_fuse_restatement as PR
from tests import orb_fuse_scenario as PS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
POINT_GOLDEN = os.path.join(ROOT, "tests", "golden", "orb_fuse_reference.npz")
LINE_GOLDEN = os.path.join(ROOT, "tests", "golden", "line_fuse_reference.npz")
ENTRIES = ("plvs_hip_keyframe_create", "plvs_hip_keyframe_destroy", "plvs_hip_keyframe_info", "plvs_hip_orb_fuse_search_kf",
           "plvs_hip_line_fuse_search_kf", "plvs_hip_fuse_search_points_and_lines_kf", "plvs_hip_orb_fuse_search_kf_host",
           "plvs_hip_line_fuse_search_kf_host")


@pytest.fixture(scope="module")
def point_golden():
    return U.point_golden(POINT_GOLDEN)


@pytest.fixture(scope="module")
def line_golden():
    return U.line_golden(LINE_GOLDEN)


@pytest.fixture(scope="module")
def point_scenario():
    return PS.inputs()


@pytest.fixture(scope="module")
def line_scenario():
    return LS.inputs()


def _points_host(inp):
    from plvs_amd.orbmatcher import ORBmatcher
    kfs, pts = PS.views(inp)
    return ORBmatcher().FuseSearch(kfs, pts, inp["th"], inp["skip"], host=True)


def _lines_host(inp):
    from plvs_amd.linematcher import LineMatcher
    kfs, lines = LS.views(inp)
    return LineMatcher().FuseSearch(kfs, lines, inp["th"], inp["skip"], host=True)


def _windows(r, first):
    return int((np.asarray(r["reached"]) >= first).sum())


# 1
def test_header_declares_and_library_exports_the_resident_entries():
    from plvs_amd import _lib
    with open(os.path.join(ROOT, "include", "plvs_hip.h")) as fh:
        header = fh.read()
    for name in ENTRIES:
        assert re.search(r"\bint " + name + r"\(", header), name
        assert hasattr(_lib.lib, name), name
    assert "typedef struct plvs_keyframe plvs_keyframe;" in header and "typedef struct plvs_keyframe_pose" in header
    assert re.search(r"#define PLVS_KEYFRAME_HOST_ONLY 1u\b", header)
    assert _lib.lib.plvs_hip_abi_version() == 1
    with open(os.path.join(ROOT, "include", "plvs_hip.hpp")) as fh:
        hpp = fh.read()
    assert "class KeyFrameHandle" in hpp and "plvs_hip_fuse_search_points_and_lines_kf" in hpp


# 2
def test_host_only_handles_equal_the_golden(point_scenario, line_scenario, point_golden, line_golden):
    out = U.search_points(point_scenario, host=True)
    U.same(out, point_golden, what="points ")
    assert out["stats"].tolist() == [0, _windows(point_golden, PR.EMPTY_WINDOW), 0, 0]
    U.same(U.search_points(PS.crowd_inputs(), host=True), {k: point_golden["crowd_" + k] for k in U.OUTPUTS}, what="point crowd ")
    out = U.search_lines(line_scenario, host=True)
    U.same(out, line_golden, what="lines ")
    assert out["stats"].tolist() == [0, _windows(line_golden, LR.EMPTY_WINDOW), 0, 0]
    U.same(U.search_lines(LS.crowd_inputs(), host=True), {k: line_golden["crowd_" + k] for k in U.OUTPUTS}, what="line crowd ")


@pytest.mark.parametrize("K", [1, 2])
@pytest.mark.parametrize("M", [1, 5])
def test_host_only_handles_equal_the_host_entries_at_other_sizes(K, M):
    for empty_kf in (None, 0):
        inp = PS.random_inputs(K, M, 80, seed=10 * K + M, empty_kf=empty_kf)
        want = _points_host(inp)
        out = U.search_points(inp, host=True)
        U.same(out, want, what=f"points empty_kf={empty_kf} ")
        assert out["stats"][:3].tolist() == want["stats"].tolist()
        inp = LS.random_inputs(K, M, 60, seed=10 * K + M, empty_kf=empty_kf)
        want = _lines_host(inp)
        out = U.search_lines(inp, host=True)
        U.same(out, want, what=f"lines empty_kf={empty_kf} ")
        assert out["stats"][:3].tolist() == want["stats"].tolist()


def _wide_theta(scenario):
    """tests/test_line_fuse.py's: key frame 1 with a scale factor of 10 at level 1, deltaTheta = 100 degrees."""
    kfs = [dict(kf) for kf in scenario["kfs"]]
    kfs[1]["scale_factors"] = np.array([1.0, 10.0, 1.44], np.float32)
    return dict(scenario, kfs=kfs)


def test_host_only_handles_on_the_ambiguous_the_degenerate_and_the_refused(line_scenario):
    from plvs_amd import _lib
    for inp in (PS.ambiguous_inputs(),):
        U.same(U.search_points(inp, host=True), _points_host(inp), what="ambiguous points ")
    for inp, what in ((LS.ambiguous_inputs(), "ambiguous lines "), (LS.degenerate_inputs(), "degenerate lines ")):
        U.same(U.search_lines(inp, host=True), _lines_host(inp), what=what)
    out = U.search_lines(LS.degenerate_inputs(), host=True)
    assert out["reached"][0, :2].tolist() == [LR.DEGENERATE, LR.DEGENERATE] and (out["best_idx"][0, :2] == -1).all()
    wide = _wide_theta(line_scenario)
    with pytest.raises(_lib.PlvsHipError) as e:
        U.search_lines(wide, host=True)
    assert e.value.code == _lib.PLVS_ERR_INVALID_ARG and "theta" in str(e.value)


# 3
def test_create_deep_copies(point_scenario, line_scenario, point_golden, line_golden):
    U.same(U.search_points(point_scenario, host=True, smash_sources=True), point_golden, what="points ")
    U.same(U.search_lines(line_scenario, host=True, smash_sources=True), line_golden, what="lines ")
    # and the overwriting does reach what a view hands to the library: the non-resident entry on the same arrays sees it
    inp = U.own_copy(point_scenario)
    kfs, pts = PS.views(inp)
    U.smash(inp, ("desc",))
    from plvs_amd.orbmatcher import ORBmatcher
    assert (ORBmatcher().FuseSearch(kfs, pts, inp["th"], inp["skip"], host=True)["best_idx"] != point_golden["best_idx"]).any()


# 4
def _refused(what, **kw):
    from plvs_amd import _lib
    from plvs_amd.keyframe import ResidentKeyFrame
    with pytest.raises(_lib.PlvsHipError) as e:
        ResidentKeyFrame(host_only=True, **kw)
    assert e.value.code == _lib.PLVS_ERR_INVALID_ARG and what in str(e.value), str(e.value)


def test_create_refuses_what_the_searches_refuse_of_a_key_frame(point_scenario, line_scenario):
    from plvs_amd.keyframe import ResidentKeyFrame
    pk, _ = PS.views(point_scenario)
    lk, _ = LS.views(line_scenario)
    rep = dataclasses.replace
    _refused("neither a point side nor a line side")
    for side, kf, pinhole in (("points", pk[0], "NLeft == -1"), ("lines", lk[1], "NlinesLeft == -1")):
        _refused(pinhole, **{side: rep(kf, n_cameras=2)})
        _refused(pinhole, **{side: rep(kf, camera_model=1)})
    # levels
    _refused("levels outside [1, 64]", points=rep(pk[0], inv_level_sigma2=np.zeros(0, np.float32)))
    _refused("levels outside [1, 64]", points=rep(pk[0], inv_level_sigma2=np.ones(65, np.float32), view=rep(pk[0].view, scale_factors=np.ones(65, np.float32))))
    many = LS.inputs()["kfs"][1]
    many["scale_factors"], many["inv_level_sigma2"] = np.ones(65, np.float32), np.ones(65, np.float32)
    _refused("line levels outside [1, 64]", lines=LS.views(dict(kfs=[many], lines=line_scenario["lines"]))[0][0])
    # an octave outside the levels
    octave = np.array(point_scenario["kfs"][0]["octave"])
    octave[3] = PS.N_LEVELS
    _refused("octave of a key point", points=rep(pk[0], view=rep(pk[0].view, octave=octave)))
    bad = dict(line_scenario["kfs"][1], kl=line_scenario["kfs"][1]["kl"].copy())
    bad["kl"]["octave"][2] = -1
    _refused("octave of a key line", lines=LS.views(dict(kfs=[bad], lines=line_scenario["lines"]))[0][0])
    # null arrays: through the C structs
    from plvs_amd import _lib
    f = _lib.lib.plvs_hip_keyframe_create
    f.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_void_p]
    h = ctypes.c_void_p()
    for field, what in (("K4", "null pose / camera array"), ("bounds4", "null pose / camera array"), ("inv_level_sigma2", "null level arrays")):
        c = pk[0].as_c()
        setattr(c, field, None)
        assert f(ctypes.byref(c), None, 1, ctypes.byref(h)) == _lib.PLVS_ERR_INVALID_ARG and not h
        assert what in _lib.lib.plvs_hip_last_error().decode()
    c = pk[0].as_c()
    c.view.desc = None
    assert f(ctypes.byref(c), None, 1, ctypes.byref(h)) == _lib.PLVS_ERR_INVALID_ARG and "null key frame array" in _lib.lib.plvs_hip_last_error().decode()
    c = lk[1].as_c()
    c.view.descriptors = None
    assert f(None, ctypes.byref(c), 1, ctypes.byref(h)) == _lib.PLVS_ERR_INVALID_ARG and "null key frame array" in _lib.lib.plvs_hip_last_error().decode()
    c = lk[2].as_c()
    c.view.u_right_end = None
    assert f(None, ctypes.byref(c), 1, ctypes.byref(h)) == _lib.PLVS_ERR_INVALID_ARG and "without the other" in _lib.lib.plvs_hip_last_error().decode()
    c = lk[1].as_c()
    c.view.max_diag = 0.0
    assert f(None, ctypes.byref(c), 1, ctypes.byref(h)) == _lib.PLVS_ERR_INVALID_ARG and "mnMaxDiag" in _lib.lib.plvs_hip_last_error().decode()
    assert f(ctypes.byref(pk[0].as_c()), None, 2, ctypes.byref(h)) == _lib.PLVS_ERR_INVALID_ARG and "unknown flag" in _lib.lib.plvs_hip_last_error().decode()
    assert _lib.lib.plvs_hip_keyframe_destroy(None) == _lib.PLVS_OK
    # the pose pointers are not read: ResidentKeyFrame hands them over as NULL, and the info is the handle's
    with ResidentKeyFrame(points=pk[0], lines=lk[1], host_only=True) as kf:
        info = kf.info()
        assert (info["n_points"], info["n_lines"], info["device_bytes"], info["flags"], info["device"]) == (len(point_scenario["kfs"][0]["x"]), LS.N_KL, 0, 1, -1)
        assert info["host_bytes"] > 32 * (info["n_points"] + info["n_lines"])


def test_searches_refuse_bad_handle_lists_before_any_device_call(point_scenario, line_scenario):
    from plvs_amd import _lib
    from plvs_amd.keyframe import (ResidentKeyFrame, fuse_search_kf, fuse_search_points_and_lines_kf, line_fuse_search_kf)
    with U.Handles(points_inp=point_scenario, host_only=True) as P, U.Handles(lines_inp=line_scenario, host_only=True) as L:
        def refused(what, f, *a, **kw):
            with pytest.raises(_lib.PlvsHipError) as e:
                f(*a, **kw)
            assert e.value.code == _lib.PLVS_ERR_INVALID_ARG and what in str(e.value), str(e.value)

        for host in (True, False):
            refused("null key-frame handle", fuse_search_kf, [P.kfs[0], None, P.kfs[2]], P.poses, P.points, host=host)
            refused("null key-frame handle", line_fuse_search_kf, [None] + L.kfs[1:], L.poses, L.lines, host=host)
            refused("without a line side", line_fuse_search_kf, P.kfs, P.poses, L.lines, host=host)
            refused("without a point side", fuse_search_kf, L.kfs, L.poses, P.points, host=host)
            refused("th outside", fuse_search_kf, P.kfs, P.poses, P.points, th=-1.0, host=host)
            refused("null output", line_fuse_search_kf, L.kfs, L.poses, L.lines, host=host, outputs=False)
        # a host-only handle in a device entry: refused before any HIP call (this machine has no device to call)
        refused("PLVS_KEYFRAME_HOST_ONLY", fuse_search_kf, P.kfs, P.poses, P.points)
        refused("PLVS_KEYFRAME_HOST_ONLY", line_fuse_search_kf, L.kfs, L.poses, L.lines)
        refused("PLVS_KEYFRAME_HOST_ONLY", fuse_search_points_and_lines_kf, P.kfs, P.poses, points=P.points)
        refused("neither points nor lines", fuse_search_points_and_lines_kf, P.kfs, P.poses)
        # nothing was written by a refused call
        out = np.full((3, P.points.as_c().m), -7, np.int32)
        f = _lib.lib.plvs_hip_orb_fuse_search_kf
        vp = ctypes.c_void_p
        f.argtypes = [vp, vp, ctypes.c_int, vp, vp, ctypes.c_float, vp, vp, vp, vp, vp]
        from plvs_amd.keyframe import _lists
        K, hs, ps = _lists(P.kfs, P.poses)
        pc = P.points.as_c()
        st = np.full(4, -1, np.int32)
        assert f(hs, ps, K, ctypes.byref(pc), None, 3.0, _lib.np_ptr(out), _lib.np_ptr(out.copy()), None, _lib.np_ptr(st), None) == _lib.PLVS_ERR_INVALID_ARG
        assert (out == -7).all() and st.tolist() == [-1] * 4
    with ResidentKeyFrame(points=PS.views(point_scenario)[0][0], host_only=True) as kf:
        kf.close()
        with pytest.raises(ValueError):
            kf.handle


def test_the_same_handle_twice_with_two_poses_on_the_host(point_scenario):
    from plvs_amd.keyframe import fuse_search_kf
    from plvs_amd.orbmatcher import ORBmatcher
    kfs, pts = PS.views(point_scenario)
    moved = dataclasses.replace(kfs[0], q_cw=kfs[1].q_cw, tcw=kfs[1].tcw, Ow=kfs[1].Ow)
    want = ORBmatcher().FuseSearch([kfs[0], moved], pts, 3.0, None, host=True)
    with U.Handles(points_inp=point_scenario, host_only=True) as h:
        out = fuse_search_kf([h.kfs[0], h.kfs[0]], [h.poses[0], h.poses[1]], h.points, 3.0, None, host=True)
    U.same(out, want)
    assert (want["best_idx"][0] != want["best_idx"][1]).any()


# 5
def run_cpp_handle_program(tmp_path, compiler, where, scenario, golden):
    """tests/host/keyframe_resident_smoke.cpp built by `compiler`, run on the host or on the device; its pairs against the golden.
    -> what it said besides the pairs."""
    from tests.test_orb_fuse import _write_pair_input
    lib_dir = os.path.join(ROOT, "plvs_amd", "lib")
    exe = str(tmp_path / "keyframe_resident_smoke")
    subprocess.run(compiler + ["-O1", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
                               os.path.join(ROOT, "tests", "host", "keyframe_resident_smoke.cpp"), "-L", lib_dir, "-l:libplvs_hip.so",
                               "-Wl,-rpath," + lib_dir, "-Wl,-rpath,/opt/rocm/lib", "-o", exe], check=True)
    path = str(tmp_path / "inputs.bin")
    _write_pair_input(path, scenario)
    r = subprocess.run([exe, path, where], capture_output=True, text=True)
    assert r.returncode == 0 and "keyframe_resident_smoke ok" in r.stdout, r.stdout[-500:] + r.stderr
    want = np.stack([golden[k].reshape(-1) for k in U.OUTPUTS], 1).astype(np.int64)
    got = np.array([[int(c) for c in ln.split()[1:]] for ln in r.stdout.splitlines() if ln.startswith("pair ")], np.int64)
    assert got.shape == want.shape and (got == want).all(), np.argwhere(got != want)[:8]
    said = {ln.split()[0]: ln.split()[1:] for ln in r.stdout.splitlines() if ln and not ln.startswith("pair ")}
    M = golden["reached"].shape[1]
    assert said["found"][:2] == [str(int((golden["best_idx"] >= 0).sum())), "stats"]
    assert said["twice"] == [str(M), "of", str(M)] and said["refused"] == ["3"]
    return said


@pytest.mark.parametrize("compiler", [["g++", "-std=c++14"], ["/opt/rocm/bin/hipcc", "-x", "c++", "-std=c++17"]])
def test_cpp_handle_on_the_host_gives_the_golden_candidates(tmp_path, compiler, point_scenario, point_golden):
    said = run_cpp_handle_program(tmp_path, compiler, "host", point_scenario, point_golden)
    assert said["found"][2:] == ["0", str(_windows(point_golden, PR.EMPTY_WINDOW)), "0", "0"]


def test_replay_over_host_only_handles_equals_the_sequential_loop():
    from tests import line_fuse_replay, orb_fuse_replay, test_line_fuse, test_orb_fuse
    for kind, P, T in (("points", orb_fuse_replay, test_orb_fuse), ("lines", line_fuse_replay, test_line_fuse)):
        inp = P.replay_inputs()
        search = U.ReplaySearcher(kind, host=True)
        try:
            assert P.replayed(inp, search).state() == P.sequential(inp, T._searcher(True)).state(), kind
        finally:
            search.close()
