"""The Fuse searches over key frames resident in HBM (plvs_hip_orb_fuse_search_kf, plvs_hip_line_fuse_search_kf,
plvs_hip_fuse_search_points_and_lines_kf) on the device.  Expected values: the compiled reference's recorded run
(tests/golden/orb_fuse_reference.npz, line_fuse_reference.npz) or the non-resident entries, which tests/test_orb_fuse.py and
tests/test_line_fuse.py pin to it — never the resident entries themselves.  Every index, distance and stage is compared for equality."""
import ctypes
import dataclasses

import numpy as np
import pytest

from tests import keyframe_resident_util as U
from tests import line_fuse_restatement as LR
from tests import line_fuse_scenario as LS
from tests import orb_fuse_restatement as PR
from tests import orb_fuse_scenario as PS
from tests.test_keyframe_resident import LINE_GOLDEN, POINT_GOLDEN, _wide_theta, run_cpp_handle_program

pytestmark = pytest.mark.gpu

# One entry of the per-call table: the pose and the constants (fusepair::KfConst: 24 floats and an int, 100 bytes; linefuse::KfConst: 28
# floats and an int, 116 bytes), padded to the pointers' alignment, then the pointers into the handle's allocation and a count
# (points: members, cell starts, u_right, descriptors, two level tables; lines: the same without u_right), padded again.
POINT_ENTRY = 104 + 6 * 8 + 8
LINE_ENTRY = 120 + 5 * 8 + 8


def up16(n):
    return (n + 15) & ~15


def point_copy_bytes(K, M, skip=True):
    return up16(K * POINT_ENTRY) + 2 * up16(12 * M) + 2 * up16(4 * M) + 32 * M + (up16(K * M) if skip else 0)


def line_copy_bytes(K, M, skip=True):
    return up16(K * LINE_ENTRY) + 3 * up16(12 * M) + up16(4 * M) + 32 * M + (up16(K * M) if skip else 0)


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


def _points(inp, kfs=None, host=False):
    """The non-resident entry (kfs: views that replace the scenario's)."""
    from plvs_amd.orbmatcher import ORBmatcher
    own, pts = PS.views(inp)
    return ORBmatcher().FuseSearch(own if kfs is None else kfs, pts, inp["th"], inp["skip"], host=host)


def _lines(inp, kfs=None, host=False):
    from plvs_amd.linematcher import LineMatcher
    own, lines = LS.views(inp)
    return LineMatcher().FuseSearch(own if kfs is None else kfs, lines, inp["th"], inp["skip"], host=host)


def _windows(r, first):
    return int((np.asarray(r["reached"]) >= first).sum())


# 6
def test_resident_equals_the_golden(point_scenario, line_scenario, point_golden, line_golden):
    out, non = U.search_points(point_scenario, host=False), _points(point_scenario)
    U.same(out, point_golden, what="points ")
    assert out["stats"][:3].tolist() == non["stats"].tolist() == [non["stats"][0], _windows(point_golden, PR.EMPTY_WINDOW), 1]
    assert out["stats"][3] == point_copy_bytes(3, point_golden["reached"].shape[1])
    out, non = U.search_lines(line_scenario, host=False), _lines(line_scenario)
    U.same(out, line_golden, what="lines ")
    assert out["stats"][:3].tolist() == non["stats"].tolist() == [non["stats"][0], _windows(line_golden, LR.EMPTY_WINDOW), 1]
    assert out["stats"][3] == line_copy_bytes(3, line_golden["reached"].shape[1])


def test_cpp_handle_on_the_device_gives_the_golden_candidates(tmp_path, point_scenario, point_golden):
    said = run_cpp_handle_program(tmp_path, ["g++", "-std=c++14"], "device", point_scenario, point_golden)
    M = point_golden["reached"].shape[1]
    assert said["found"][3:] == [str(_windows(point_golden, PR.EMPTY_WINDOW)), "1", str(point_copy_bytes(3, M))]


# 7
def test_resident_crowds_turn_the_stride_loop(point_golden, line_golden):
    crowd = PS.crowd_inputs(200)
    assert len(crowd["kfs"][0]["x"]) == 200
    U.same(U.search_points(crowd, host=False), {k: point_golden["crowd_" + k] for k in U.OUTPUTS}, what="points ")
    crowd = LS.crowd_inputs(150)
    assert len(LR.grid_of(crowd["kfs"][0])[1]) > 128
    U.same(U.search_lines(crowd, host=False), {k: line_golden["crowd_" + k] for k in U.OUTPUTS}, what="lines ")


# 8
@pytest.mark.parametrize("K", [1, 2])
@pytest.mark.parametrize("M", [1, 3, 4, 5])
def test_resident_workgroup_edges(K, M):
    """Four pairs per workgroup: 1, 3, 4, 5 and 8 pairs (and 2, 6, 10)."""
    inp = PS.random_inputs(K, M, 120, seed=M)
    want, out = _points(inp), U.search_points(inp, host=False)
    U.same(out, want, what="points ")
    assert out["stats"][:3].tolist() == want["stats"].tolist() and out["stats"][3] == point_copy_bytes(K, M)
    inp = LS.random_inputs(K, M, 120, seed=M)
    want, out = _lines(inp), U.search_lines(inp, host=False)
    U.same(out, want, what="lines ")
    assert out["stats"][:3].tolist() == want["stats"].tolist() and out["stats"][3] == line_copy_bytes(K, M)


def test_resident_empty_key_frame_among_others_and_every_pair_skipped():
    for S, search, non, R in ((PS, U.search_points, _points, PR), (LS, U.search_lines, _lines, LR)):
        inp = S.random_inputs(3, 9, 100, seed=3, empty_kf=1)
        want, out = non(inp), search(inp, host=False)
        U.same(out, want)
        assert out["stats"][:3].tolist() == want["stats"].tolist() and out["stats"][2] == 1
        assert (out["reached"][1] <= R.EMPTY_WINDOW).all()
        inp["skip"] = np.ones_like(inp["skip"])
        out = search(inp, host=False)
        assert out["stats"].tolist() == [0, 0, 0, 0] and (out["reached"] == R.SKIPPED).all() and (out["best_idx"] == -1).all()
        # no key frame, no item, no key frame with features: nothing is launched, every pair reported from the host's code
        for shape in (S.random_inputs(0, 7, 40, seed=4), S.random_inputs(2, 0, 40, seed=4), S.random_inputs(2, 7, 0, seed=4)):
            want, out = non(shape, host=True), search(shape, host=False)
            U.same(out, want)
            assert out["stats"][2] == 0 and out["stats"][3] == 0


# 9
def test_the_pose_is_the_calls():
    from plvs_amd.keyframe import KeyFramePose, fuse_search_kf, line_fuse_search_kf
    rep = dataclasses.replace
    pin, lin = PS.random_inputs(3, 40, 150, seed=9), LS.random_inputs(3, 40, 100, seed=9)
    pk, pts = PS.views(pin)
    lk, lines = LS.views(lin)
    with U.Handles(points_inp=pin) as P, U.Handles(lines_inp=lin) as L:
        for shift in (0, 1):        # the key frames' own poses, then each key frame with its neighbour's
            order = [(k + shift) % 3 for k in range(3)]
            moved = [rep(pk[k], q_cw=pk[j].q_cw, tcw=pk[j].tcw, Ow=pk[j].Ow) for k, j in enumerate(order)]
            U.same(fuse_search_kf(P.kfs, [P.poses[j] for j in order], pts, pin["th"], pin["skip"]), _points(pin, moved), what=f"points shift {shift} ")
            moved = [rep(lk[k], Rcw=lk[j].Rcw, tcw=lk[j].tcw, Ow=lk[j].Ow) for k, j in enumerate(order)]
            U.same(line_fuse_search_kf(L.kfs, [L.poses[j] for j in order], lines, lin["th"], lin["skip"]), _lines(lin, moved), what=f"lines shift {shift} ")
        # one handle twice in one call with two poses; the list reversed; a subset
        twice = [rep(pk[0]), rep(pk[0], q_cw=pk[2].q_cw, tcw=pk[2].tcw, Ow=pk[2].Ow)]
        sk = pin["skip"][[0, 0]]
        from plvs_amd.orbmatcher import ORBmatcher
        want = ORBmatcher().FuseSearch(twice, pts, pin["th"], sk)
        U.same(fuse_search_kf([P.kfs[0], P.kfs[0]], [P.poses[0], P.poses[2]], pts, pin["th"], sk), want, what="twice ")
        assert (want["reached"][0] != want["reached"][1]).any()
        from plvs_amd.linematcher import LineMatcher
        twice = [rep(lk[1]), rep(lk[1], Rcw=lk[0].Rcw, tcw=lk[0].tcw, Ow=lk[0].Ow)]
        sk = lin["skip"][[1, 1]]
        want = LineMatcher().FuseSearch(twice, lines, lin["th"], sk)
        U.same(line_fuse_search_kf([L.kfs[1], L.kfs[1]], [L.poses[1], L.poses[0]], lines, lin["th"], sk), want, what="twice, lines ")
        for order in ([2, 1, 0], [2, 0]):
            want = ORBmatcher().FuseSearch([pk[k] for k in order], pts, pin["th"], pin["skip"][order])
            U.same(fuse_search_kf([P.kfs[k] for k in order], [P.poses[k] for k in order], pts, pin["th"], pin["skip"][order]), want, what=f"points {order} ")
            want = LineMatcher().FuseSearch([lk[k] for k in order], lines, lin["th"], lin["skip"][order])
            U.same(line_fuse_search_kf([L.kfs[k] for k in order], [L.poses[k] for k in order], lines, lin["th"], lin["skip"][order]), want, what=f"lines {order} ")
    assert isinstance(P.poses[0], KeyFramePose)


# 10
def test_residency_is_real():
    """The call's copy in holds the table, the items and skip — computed here from K and M — whatever the key frames hold, and the
    arrays the handles were made from are gone before the search."""
    K, M = 3, 37
    for S, search, non, nbytes in ((PS, U.search_points, _points, point_copy_bytes), (LS, U.search_lines, _lines, line_copy_bytes)):
        seen = []
        for N in (50, 400):
            inp = S.random_inputs(K, M, N, seed=6)
            want = non(inp)
            out = search(inp, host=False, smash_sources=True)
            U.same(out, want, what=f"N = {N} ")
            assert out["stats"][:3].tolist() == want["stats"].tolist()
            seen.append(int(out["stats"][3]))
        assert seen == [nbytes(K, M)] * 2
        inp["skip"] = None
        assert search(inp, host=False)["stats"][3] == nbytes(K, M, skip=False)


# 11
def test_resident_ambiguous_pairs_go_through_the_host_copy():
    inp = PS.ambiguous_inputs()
    want, out = _points(inp), U.search_points(inp, host=False, smash_sources=True)
    assert out["stats"][0] == want["stats"][0] > 0
    U.same(out, want, what="points ")
    U.same(out, _points(inp, host=True), what="points, host ")
    inp = LS.ambiguous_inputs()
    want, out = _lines(inp), U.search_lines(inp, host=False, smash_sources=True)
    assert out["stats"][0] == want["stats"][0] >= 13
    U.same(out, want, what="lines ")
    U.same(out, _lines(inp, host=True), what="lines, host ")


# 12
def test_resident_degenerate_lines_and_the_theta_refusal(point_scenario, line_scenario, point_golden):
    from plvs_amd import _lib
    from plvs_amd.keyframe import _lists
    inp = LS.degenerate_inputs()
    out = U.search_lines(inp, host=False)
    U.same(out, _lines(inp), what="degenerate ")
    assert out["reached"][0, :2].tolist() == [LR.DEGENERATE, LR.DEGENERATE]
    wide = _wide_theta(line_scenario)
    with pytest.raises(_lib.PlvsHipError) as e:
        _lines(wide)
    assert "theta" in str(e.value)
    with pytest.raises(_lib.PlvsHipError) as e:
        U.search_lines(wide, host=False)
    assert e.value.code == _lib.PLVS_ERR_INVALID_ARG and "theta" in str(e.value)
    # the combined entry: the refusal leaves the line outputs untouched, the point outputs are in place
    with U.Handles(points_inp=point_scenario, lines_inp=wide) as h:
        K, hs, ps = _lists(h.kfs, h.poses)
        pc, lc = h.points.as_c(), h.lines.as_c()
        mk = lambda m: (np.full((K, m), -7, np.int32), np.full((K, m), -7, np.int32), np.full((K, m), 255, np.uint8), np.full(4, -1, np.int32))
        po, lo = mk(pc.m), mk(lc.m)
        psk, lsk = np.ascontiguousarray(point_scenario["skip"], np.uint8), np.ascontiguousarray(wide["skip"], np.uint8)
        st = np.full(3, -1, np.int32)
        f = _lib.lib.plvs_hip_fuse_search_points_and_lines_kf
        vp, fl = ctypes.c_void_p, ctypes.c_float
        f.argtypes = [vp, vp, ctypes.c_int, vp, vp, fl, vp, vp, vp, vp, vp, vp, fl, vp, vp, vp, vp, vp, vp]
        rc = f(hs, ps, K, ctypes.byref(pc), _lib.np_ptr(psk), 3.0, *[_lib.np_ptr(a) for a in po], ctypes.byref(lc), _lib.np_ptr(lsk), 3.0,
               *[_lib.np_ptr(a) for a in lo], _lib.np_ptr(st), None)
        assert rc == _lib.PLVS_ERR_INVALID_ARG and "theta" in _lib.lib.plvs_hip_last_error().decode()
        assert (lo[0] == -7).all() and (lo[1] == -7).all() and (lo[2] == 255).all()
        pk, lk = PS.views(point_scenario)[0], LS.views(wide)[0]
        moved = [dataclasses.replace(pk[k], tcw=lk[k].tcw, Ow=lk[k].Ow) for k in range(3)]
        U.same(dict(best_idx=po[0], best_dist=po[1], reached=po[2]), _points(point_scenario, moved), what="points of the refused call ")
        U.same(dict(best_idx=po[0][:1]), dict(best_idx=point_golden["best_idx"][:1]), keys=("best_idx",), what="key frame 0 keeps its pose ")


# 13
def test_combined_entry_equals_the_two_entries_after_one_wait(point_scenario, line_scenario, point_golden, line_golden):
    """ONE key-frame list for both kinds: handle k holds point key frame k and line key frame k, and pose k is one pose — the line
    scenario's translation and centre go with the point scenario's quaternion, so the points are held against the non-resident point
    entry at that pose (key frame 0, with the placed cases, has the same pose in both scenarios) and the lines against the golden."""
    from plvs_amd.keyframe import fuse_search_kf, fuse_search_points_and_lines_kf, line_fuse_search_kf
    pk, _ = PS.views(point_scenario)
    lk, _ = LS.views(line_scenario)
    moved = [dataclasses.replace(pk[k], tcw=lk[k].tcw, Ow=lk[k].Ow) for k in range(3)]
    want_p, want_l = _points(point_scenario, moved), _lines(line_scenario)
    U.same(want_l, line_golden)
    assert (want_p["best_idx"][0] == point_golden["best_idx"][0]).all() and _windows(want_p, PR.CANDIDATE) > 20
    with U.Handles(points_inp=point_scenario, lines_inp=line_scenario) as h:
        info = h.kfs[1].info()
        assert (info["n_points"], info["n_lines"]) == (PS.N_KP, LS.N_KL)
        args = dict(points=h.points, th_points=3.0, skip_points=point_scenario["skip"], lines=h.lines, th_lines=3.0, skip_lines=line_scenario["skip"])
        p, l, stats = fuse_search_points_and_lines_kf(h.kfs, h.poses, **args)
        U.same(p, want_p, what="points ")
        U.same(l, want_l, what="lines ")
        one_p = fuse_search_kf(h.kfs, h.poses, h.points, 3.0, point_scenario["skip"])
        one_l = line_fuse_search_kf(h.kfs, h.poses, h.lines, 3.0, line_scenario["skip"])
        U.same(p, one_p, what="points, single ")
        U.same(l, one_l, what="lines, single ")
        assert p["stats"].tolist() == one_p["stats"].tolist() and l["stats"].tolist() == one_l["stats"].tolist()
        assert p["stats"][:3].tolist() == want_p["stats"].tolist() and l["stats"][:3].tolist() == want_l["stats"].tolist()
        M_p, M_l = want_p["reached"].shape[1], want_l["reached"].shape[1]
        assert stats.tolist() == [2, 1, point_copy_bytes(3, M_p) + line_copy_bytes(3, M_l)]
        p, l, stats = fuse_search_points_and_lines_kf(h.kfs, h.poses, **{k: v for k, v in args.items() if "lines" not in k})
        assert l is None and stats.tolist() == [1, 1, point_copy_bytes(3, M_p)]
        U.same(p, want_p, what="points alone ")
        p, l, stats = fuse_search_points_and_lines_kf(h.kfs, h.poses, **{k: v for k, v in args.items() if "points" not in k})
        assert p is None and stats.tolist() == [1, 1, line_copy_bytes(3, M_l)]
        U.same(l, want_l, what="lines alone ")
    # a points-only handle in the combined call, with device handles: the line side is missed before anything is launched
    from plvs_amd import _lib
    with U.Handles(points_inp=point_scenario) as h:
        with pytest.raises(_lib.PlvsHipError) as e:
            fuse_search_points_and_lines_kf(h.kfs, h.poses, **args)
        assert "without a line side" in str(e.value)


# 14
def test_replay_over_resident_key_frames_equals_the_sequential_loop():
    from tests import line_fuse_replay, orb_fuse_replay, test_line_fuse, test_orb_fuse
    for kind, P, T in (("points", orb_fuse_replay, test_orb_fuse), ("lines", line_fuse_replay, test_line_fuse)):
        inp = P.replay_inputs()
        want = P.sequential(inp, T._searcher(True))
        batch, requery = U.ReplaySearcher(kind, host=False), U.ReplaySearcher(kind, host=True)
        try:
            log = []
            got = P.replayed(inp, requery, batch_search=batch, log=log)
            assert got.state() == want.state(), kind
            assert any(stale != live for _, _, stale, live in log), "no dirty item whose stale candidate differs from its live one"
        finally:
            batch.close()
            requery.close()


# 15
def test_life_cycle():
    from plvs_amd import _lib
    from plvs_amd.keyframe import ResidentKeyFrame, fuse_search_kf, pose_of
    inp = PS.random_inputs(1, 12, 90, seed=15)
    (view,), pts = PS.views(inp)
    want = _points(inp)
    made = [ResidentKeyFrame(points=view) for _ in range(64)]
    # the device bytes are what the arrays add up to: members (16 N), cell starts (64 x 48 + 1 ints), u_right (4 N), descriptors (32 N)
    # and two level tables, each from a multiple of 16
    info = made[0].info()
    N, levels = 90, PS.N_LEVELS
    assert info["device_bytes"] == info["host_bytes"] == up16(16 * N) + up16(4 * (64 * 48 + 1)) + up16(4 * N) + 32 * N + up16(4 * levels) + 4 * levels
    assert info["device"] >= 0 and info["flags"] == 0
    for kf in made[::2]:
        kf.close()
    survivors = made[1::2]
    out = fuse_search_kf(survivors, [pose_of(points=view)] * 32, pts, inp["th"], np.repeat(inp["skip"], 32, 0))
    for k in range(32):
        U.same({n: out[n][k:k + 1] for n in U.OUTPUTS}, want, what=f"survivor {k} ")
    for kf in survivors:
        kf.close()
    with pytest.raises(_lib.PlvsHipError):       # a closed handle never reaches the library
        fuse_search_kf([None], [pose_of(points=view)], pts)


def test_a_handle_from_another_device_is_refused():
    from plvs_amd import _lib
    from plvs_amd.keyframe import ResidentKeyFrame, fuse_search_kf, pose_of
    n = ctypes.c_int()
    _lib.check(_lib.lib.plvs_hip_device_count(ctypes.byref(n)))
    if n.value < 2:
        pytest.skip(f"needs two devices to create a handle on one and search on the other: plvs_hip_device_count() == {n.value}")
    inp = PS.random_inputs(1, 5, 60, seed=16)
    (view,), pts = PS.views(inp)
    _lib.check(_lib.lib.plvs_hip_set_device(1))
    try:
        kf = ResidentKeyFrame(points=view)
    finally:
        _lib.check(_lib.lib.plvs_hip_set_device(0))
    with pytest.raises(_lib.PlvsHipError) as e:
        fuse_search_kf([kf], [pose_of(points=view)], pts)
    assert "another device" in str(e.value)
    kf.close()
