"""ORBmatcher::SearchByBoW over resident key frames (plvs_hip_keyframe_create_bow, plvs_hip_orb_search_by_bow_kf,
plvs_hip_orb_search_by_bow_frame_kf and the two _kf_host entries) against the compiled reference's recorded run
(tests/golden/bow_search_reference.npz, scripts/make_bow_search_golden.py) and, at other sizes, against the restatement that the golden
pins (tests/bow_search_restatement.py).  Every comparison is for equality."""
import ctypes
import json
import os
import re

import numpy as np
import pytest

from tests import bow_search_restatement as R
from tests import bow_search_scenario as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "bow_search_reference.npz")
FACTS = os.path.join(ROOT, "tests", "golden", "bow_search_reference_facts.json")
ENTRIES = ("plvs_hip_keyframe_create_bow", "plvs_hip_keyframe_bow_info", "plvs_hip_orb_search_by_bow_kf", "plvs_hip_orb_search_by_bow_frame_kf",
           "plvs_hip_orb_search_by_bow_kf_host", "plvs_hip_orb_search_by_bow_frame_kf_host")
KINDS = (R.KF, R.FRAME)


@pytest.fixture(scope="module", autouse=True)
def entries_exist():
    """Every test here is about these entries: without them the first missing symbol fails it."""
    from plvs_amd import _lib
    for name in ENTRIES:
        assert hasattr(_lib.lib, name), name


@pytest.fixture(scope="module")
def facts():
    with open(FACTS) as fh:
        return json.load(fh)


@pytest.fixture(scope="module")
def golden():
    return dict(np.load(GOLDEN))


def want_of(golden, cname, kind, run):
    """The entries' outputs of a call as the golden holds them: (match [K,n_A], match_dist [K,n_A], nmatches [K])."""
    a_side, b_sides = S.calls()[cname]
    pre = f"{cname}_{kind}_{run}_"
    shape = (len(b_sides), len(a_side["desc"]))
    return golden[pre + "match"].astype(np.int32).reshape(shape), golden[pre + "match_dist"].astype(np.int32).reshape(shape), golden[pre + "nmatches"]


class Handles:
    """The handles of one scenario call: `a` for the A side, `bs` for the key frames.  A side that is listed twice (the degenerate
    call's partner) is ONE handle listed twice."""

    def __init__(self, a_side, b_sides, host_only):
        self.a_side, self.b_sides = a_side, b_sides
        self.a = S.key_frame(a_side, host_only)
        made = {}
        for b in b_sides:
            if id(b) not in made:
                made[id(b)] = S.key_frame(b, host_only)
        self.bs = [made[id(b)] for b in b_sides]

    def close(self):
        for h in [self.a] + self.bs:
            h.close()          # (closing a handle twice is a no-op)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


def search(h, kind, ratio, ori, host, bs=None, b_sides=None, **kw):
    """-> (match, match_dist, nmatches, stats) of the kind's entry over the handles."""
    from plvs_amd.keyframe import search_by_bow_frame_kf, search_by_bow_kf
    bs = h.bs if bs is None else bs
    b_sides = h.b_sides if b_sides is None else b_sides
    valid = [S.valid_of(b) for b in b_sides]
    if kind == R.KF:
        r = search_by_bow_kf(h.a, S.valid_of(h.a_side), bs, valid, ratio, ori, host=host, **kw)
        return r["match_idx"], r["match_dist"], r["nmatches"], r["stats"]
    r = search_by_bow_frame_kf(bs, valid, S.bow_frame(h.a_side), ratio, ori, host=host, **kw)
    return r["assigned"], r["match_dist"], r["nmatches"], r["stats"]


def equal(got, want, what):
    for name, a, b in zip(("match", "match_dist", "nmatches"), got, want):
        a, b = np.asarray(a), np.asarray(b)
        assert a.shape == b.shape and (a == b).all(), f"{what}: {name} differs at {np.argwhere(a != b)[:8].tolist()}"


def check_call_against_golden(golden, cname, host, twice=False):
    a_side, b_sides = S.calls()[cname]
    stats = {}
    with Handles(a_side, b_sides, host_only=host) as h:
        for kind in KINDS:
            for run, ratio, ori in S.RUNS:
                for rep in range(2 if twice else 1):          # the handles reused across calls
                    m, d, n, st = search(h, kind, ratio, ori, host)
                    equal((m, d, n), want_of(golden, cname, kind, run), f"{cname} {kind} {run} rep {rep}")
                stats[kind, run] = st
    return stats


# ---------------------------------------------------------------------------------------------------------------- the pin
def test_scenario_digests_match_the_golden(facts):
    assert S.digests() == facts["digests"]
    assert [list(r) for r in S.RUNS] == facts["runs"]


def test_restatement_equals_the_golden(golden, facts):
    for cname, (a_side, b_sides) in S.calls().items():
        for kind in KINDS:
            for run, ratio, ori in S.RUNS:
                counts = {}
                match, dist, n, per_k = R.search_call(a_side, b_sides, kind, ratio, ori, counts)
                equal((match, dist, n), want_of(golden, cname, kind, run), f"{cname} {kind} {run}")
                pre = f"{cname}_{kind}_{run}_"
                for key in ("best1", "best2", "raw_idx", "n_dist", "raw_bin", "cut"):
                    got = np.concatenate([np.asarray(r[key]).astype(np.int16) for r in per_k])
                    assert (got == golden[pre + key]).all(), f"{pre}{key}"
                want = facts["counts"][f"{cname}_{kind}_{run}"]
                assert {k: (v if isinstance(v, list) else int(v)) for k, v in counts.items()} == want


def test_golden_run_takes_every_placed_case(golden, facts):
    """The cap is zero: no placed case may be missing from the reference's recorded run."""
    _, where = S.scenario()
    assert facts["where"] == json.loads(json.dumps(where))
    a_side, b_sides = S.calls()["main"]
    n_a = len(a_side["desc"])
    for kind in KINDS:
        lens = [n_a if kind == R.KF else len(b["desc"]) for b in b_sides]

        def q(name, run, key, which=0):
            w = where[f"{name}_{kind}"]
            at = int(np.sum(lens[:w["k"]]))
            return int(golden[f"main_{kind}_{run}_{key}"][at + w["queries"][which]])

        def matched(name, run):
            w = where[f"{name}_{kind}"]
            row = golden[f"main_{kind}_{run}_match"][w["k"] * n_a:(w["k"] + 1) * n_a]
            return bool(row[w["queries"][0]] >= 0) if kind == R.KF else bool((row == w["queries"][0]).any())

        lo, hi, mid = "r075_ori", "r15_plain", "r09_ori"
        assert q("single_member", lo, "best2") == 256 and matched("single_member", lo)
        for name, first in (("equal_minima", 0), ("tie_descending", 1)):
            m = where[f"{name}_{kind}"]["members"]
            assert q(name, lo, "best1") == q(name, lo, "best2") == 30 and q(name, hi, "raw_idx") == m[first]
            assert not matched(name, lo) and matched(name, hi)
        m = where[f"tie_descending_{kind}"]["members"]
        assert m[1] > m[0], "the tie's winner is the higher feature index"
        m = where[f"second_taken_{kind}"]["members"]
        assert [q("second_taken", lo, "raw_idx", i) for i in (0, 1)] == m and q("second_taken", lo, "best1", 1) == 27
        assert q("all_closed", lo, "best1", 1) == 256 and q("all_closed", lo, "n_dist", 1) == 0 and q("all_closed", lo, "raw_idx", 0) >= 0
        assert [q(f"at_{b}", lo, "best1") for b in (49, 50, 51)] == [49, 50, 51]
        assert [matched(f"at_{b}", lo) for b in (49, 50, 51)] == [True, kind == R.FRAME, False]
        assert (q("ratio_equal", lo, "best1"), q("ratio_equal", lo, "best2")) == (30, 40)
        assert np.float32(30) == np.float32(0.75) * np.float32(40) and not matched("ratio_equal", lo) and matched("ratio_equal", mid)
        assert q("bin_12", lo, "raw_bin") == 12
        c = facts["counts"][f"main_{kind}_{lo}"]
        for key in ("best2_stays_256", "best1_stays_256_all_closed", "equal_minima", "tie_winner_not_lowest_index", "took_behind_a_closed_best",
                    "best1_at_th_low", "ratio_at_equality", "bin_12", "bin_tie_at_cut", "serial_list_of_1", "cut_by_rotation", "multi_pass_jobs"):
            assert c[key] >= 1, (kind, key)
        assert (c["best1_at_th_low_accepted"] >= 1) == (kind == R.FRAME)
        assert {1, 2, 63, 64, 65} | ({129} if kind == R.KF else set()) <= set(c["lane_lengths"])
        assert facts["counts"][f"degenerate_{kind}_{lo}"]["lane_lengths"] == [200]       # the frame kind's list beyond one pass
        nm = golden[f"main_{kind}_{lo}_nmatches"]
        assert nm[where["no_common_node"]["k"]] == 0 and nm[where["all_invalid"]["k"]] == 0 and nm[where["bin_tie"]["k"]] == 7
        assert facts["counts"][f"main_{kind}_{hi}"]["cut_by_rotation"] == 0              # check_orientation 0
        assert golden[f"degenerate_{kind}_{lo}_nmatches"][1] == 0                        # the key frame with an empty vector


# ---------------------------------------------------------------------------------------------------------------- host twins
@pytest.mark.parametrize("cname", ["main", "degenerate"])
def test_host_entries_equal_the_golden(golden, cname):
    stats = check_call_against_golden(golden, cname, host=True)
    for st in stats.values():
        assert st[0] == st[1] == st[2] == st[5] == 0 and st[3] > 0


@pytest.mark.parametrize("seed,shape", [(5, (130, 90, 3, 9)), (6, (60, 250, 2, 3)), (7, (1, 40, 2, 1))])
def test_host_entries_equal_the_restatement_at_other_sizes(seed, shape):
    a_side, b_sides = S.random_sides(seed, *shape)
    with Handles(a_side, b_sides, host_only=True) as h:
        for kind in KINDS:
            for run, ratio, ori in S.RUNS:
                equal(search(h, kind, ratio, ori, True)[:3], R.search_call(a_side, b_sides, kind, ratio, ori)[:3], f"seed {seed} {kind} {run}")


def test_frame_kind_at_k1_equals_the_compiled_reference_matcher():
    """Where oracle/_ref/libmatchers_ref.so is built: the reference's own SearchByBoW(pKF, F) through the oracle's wrapper."""
    path = os.path.join(ROOT, "oracle", "_ref", "libmatchers_ref.so")
    if not os.path.exists(path):
        pytest.skip("oracle/_ref/libmatchers_ref.so is not built")
    ref = ctypes.CDLL(path)
    _vp, _i, _f = ctypes.c_void_p, ctypes.c_int, ctypes.c_float
    fn = ref.ref_orb_search_by_bow
    fn.argtypes = [_vp, _vp, _i, _vp, _vp, _vp, _vp, _i, _vp, _f, _i, _vp]
    fn.restype = _i
    a_side, b_sides = S.random_sides(8, 140, 160, 2, 10)
    p = lambda a: a.ctypes.data_as(_vp)
    with Handles(a_side, b_sides, host_only=True) as h:
        for k, b in enumerate(b_sides):
            kv, fv = S.feature_vector(b), S.feature_vector(a_side)
            kc, fc = kv.as_c(), fv.as_c()
            kd, fd, valid = np.ascontiguousarray(b["desc"]), np.ascontiguousarray(a_side["desc"]), S.valid_of(b)
            want = np.full(len(fd), -9, np.int32)
            want_n = fn(ctypes.byref(kc), p(kd), len(kd), p(valid), p(b["angle"]), ctypes.byref(fc), p(fd), len(fd), p(a_side["angle"]), 0.75, 1, p(want))
            m, d, n, _ = search(h, R.FRAME, 0.75, 1, True, bs=[h.bs[k]], b_sides=[b])
            assert n[0] == want_n > 10 and (m[0] == want).all()


# ---------------------------------------------------------------------------------------------------------------- handles, refusals
def test_create_bow_info_and_the_plain_create():
    from plvs_amd.keyframe import ResidentKeyFrame
    s, _ = S.scenario()
    side = s["A0"]
    with S.key_frame(side, host_only=True) as kf, ResidentKeyFrame(points=S.point_side(side), host_only=True) as plain:
        lens = [len(v) for v in side["nodes"].values()]
        assert kf.bow_info() == dict(nodes=len(lens), listed=sum(lens), longest=max(lens), device_bytes=0)
        assert plain.bow_info()["nodes"] == -1
        a, b = kf.info(), plain.info()
        assert a["n_points"] == b["n_points"] == len(side["desc"]) and a["device_bytes"] == b["device_bytes"] == 0
        assert a["host_bytes"] > b["host_bytes"]


def _refused(call):
    from plvs_amd._lib import PlvsHipError
    with pytest.raises(PlvsHipError):
        call()


def test_create_refuses_a_bad_vector_before_anything_else():
    from plvs_amd.keyframe import KeyFrameBow, ResidentKeyFrame
    from plvs_amd.orbmatcher import FeatureVector
    s, _ = S.scenario()
    side = s["B"][0]
    n = len(side["desc"])
    good = S.feature_vector(side)

    def vec(node_id=None, offset=None, index=None):
        v = FeatureVector({})
        v.node_id = good.node_id.copy() if node_id is None else np.ascontiguousarray(node_id, np.uint32)
        v.offset = good.offset.copy() if offset is None else np.asarray(offset, np.int32)
        v.index = good.index.copy() if index is None else np.asarray(index, np.uint32)
        return v

    ids = good.node_id.copy()
    ids[1] = ids[0]
    off = good.offset.copy()
    off[1], off[2] = off[2], off[1] if off[1] != off[2] else off[1] - 1
    big, dup = good.index.copy(), good.index.copy()
    big[0] = n
    dup[-1] = dup[0]
    for bad in (vec(node_id=ids), vec(node_id=good.node_id[::-1]), vec(offset=off), vec(index=big), vec(index=dup)):
        _refused(lambda: S.key_frame(side, host_only=True, vec=bad))
        _refused(lambda: S.key_frame(side, host_only=False, vec=bad))           # before any HIP call: refused without a device too
    _refused(lambda: S.key_frame(side, host_only=True, angle=None))
    _refused(lambda: ResidentKeyFrame(points=None, bow=KeyFrameBow(good, side["angle"]), host_only=True))      # bow needs the point side
    # the frame's vector gets the same checks
    with Handles(s["A0"], [side], host_only=True) as h:
        from plvs_amd.keyframe import search_by_bow_frame_kf
        for bad in (vec(node_id=ids), vec(offset=off), vec(index=big), vec(index=dup)):
            out = (np.full((1, n), -5, np.int32), np.full((1, n), -5, np.int32), np.full(1, -5, np.int32), np.full(6, -5, np.int32))
            _refused(lambda: search_by_bow_frame_kf([h.bs[0]], [S.valid_of(side)], S.bow_frame(side, vec=bad), host=True, outputs=out))
            assert all((o == -5).all() for o in out)


def test_entries_refuse_and_leave_the_outputs_untouched():
    from plvs_amd.keyframe import ResidentKeyFrame, search_by_bow_frame_kf, search_by_bow_kf
    s, _ = S.scenario()
    a_side, b = s["A0"], s["B"][0]
    n_a = len(a_side["desc"])
    with Handles(a_side, [b], host_only=True) as h, ResidentKeyFrame(points=S.point_side(b), host_only=True) as plain:
        va, vb = S.valid_of(a_side), S.valid_of(b)
        frame = S.bow_frame(a_side)

        def both(bs, ratio, host, a=h.a):
            for kind in KINDS:
                out = (np.full((len(bs), n_a), -5, np.int32), np.full((len(bs), n_a), -5, np.int32), np.full(len(bs), -5, np.int32), np.full(6, -5, np.int32))
                if kind == R.KF:
                    _refused(lambda: search_by_bow_kf(a, va, bs, [vb] * len(bs), ratio, 1, host=host, n1=n_a, outputs=out))
                else:
                    _refused(lambda: search_by_bow_frame_kf(bs, [vb] * len(bs), frame, ratio, 1, host=host, outputs=out))
                assert all((o == -5).all() for o in out), kind

        both([h.bs[0], None], 0.75, True)                 # a NULL handle
        both([plain], 0.75, True)                         # a handle without a BoW side
        both([h.bs[0]], -0.5, True)                       # nn_ratio negative
        both([h.bs[0]], float("nan"), True)               # nn_ratio NaN
        both([h.bs[0]], 0.75, False)                      # a host-only handle on a device entry: refused before any HIP call
        out = (np.full((1, n_a), -5, np.int32), np.full((1, n_a), -5, np.int32), np.full(1, -5, np.int32), np.full(6, -5, np.int32))
        _refused(lambda: search_by_bow_kf(None, va, [h.bs[0]], [vb], 0.75, 1, host=True, n1=n_a, outputs=out))      # a NULL kf1
        _refused(lambda: search_by_bow_kf(plain, vb, [h.bs[0]], [vb], 0.75, 1, host=True, n1=n_a, outputs=out))     # kf1 without a BoW side
        assert all((o == -5).all() for o in out)


def test_host_launch_free_shapes_return_zeros():
    from plvs_amd.keyframe import search_by_bow_frame_kf, search_by_bow_kf
    s, where = S.scenario()
    a_side = s["A0"]
    with Handles(a_side, [s["B"][where["no_common_node"]["k"]], s["B"][where["all_invalid"]["k"]], s["empty"]], host_only=True) as h:
        for kind in KINDS:
            m, d, n, st = search(h, kind, 0.75, 1, True)
            assert (m == -1).all() and (d == -1).all() and (n == 0).all() and st.tolist()[:3] == [0, 0, 0] and st[5] == 0
        r = search_by_bow_kf(h.a, S.valid_of(a_side), [], [], host=True)
        assert r["match_idx"].shape == (0, len(a_side["desc"])) and r["stats"].tolist() == [0] * 6
        r = search_by_bow_frame_kf([], [], S.bow_frame(a_side), host=True)
        assert r["stats"].tolist() == [0] * 6


def test_header_declares_and_library_exports_the_entries():
    from plvs_amd import _lib
    with open(os.path.join(ROOT, "include", "plvs_hip.h")) as fh:
        text = fh.read()
    for name in ENTRIES:
        assert re.search(r"\bint " + name + r"\(", text), name
        assert hasattr(_lib.lib, name)
    assert "typedef struct plvs_keyframe_bow" in text and "typedef struct plvs_bow_frame" in text
    _lib.lib.plvs_hip_abi_version.restype = ctypes.c_int
    assert _lib.lib.plvs_hip_abi_version() == 1


# ---------------------------------------------------------------------------------------------------------------- the device
@pytest.mark.gpu
@pytest.mark.parametrize("cname", ["main", "degenerate"])
def test_device_entries_equal_the_golden_with_the_handles_reused(golden, cname):
    """Both kinds, every run, each call made twice over the same handles; `degenerate` lists the same handle twice."""
    a_side, b_sides = S.calls()[cname]
    stats = check_call_against_golden(golden, cname, host=False, twice=True)
    for (kind, run), st in stats.items():
        assert st[0] == 1 and st[1] == 1 and st[2] > 0 and st[5] == 0, (kind, run, st)
        assert st[4] > 0                                   # lists of 65 and 129 (main), of 200 (degenerate): more than one pass of 64 lanes
        counts = {}
        R.search_call(a_side, b_sides, kind, 0.75, 1, counts)
        assert st[3] == counts["common_nodes"] and st[4] == counts["multi_pass_jobs"]


@pytest.mark.gpu
def test_device_the_same_handle_listed_twice_and_as_both_sides(golden):
    s, _ = S.scenario()
    a_side = s["A0"]
    sides = [s["B"][3], s["B"][3], a_side]
    with Handles(a_side, sides, host_only=False) as h:
        bs = [h.bs[0], h.bs[0], h.a]                       # one handle twice, and kf1 itself among its partners
        for kind in KINDS:
            got = search(h, kind, 0.9, 1, False, bs=bs)
            want = R.search_call(a_side, sides, kind, 0.9, 1)[:3]
            equal(got[:3], want, kind)
            assert (got[0][0] == got[0][1]).all() and got[2][2] > 50       # a key frame against itself: most features match


@pytest.mark.gpu
@pytest.mark.parametrize("seed,shape", [(5, (130, 90, 3, 9)), (6, (60, 250, 2, 3)), (9, (300, 300, 5, 2))])
def test_device_equals_the_restatement_and_the_host_twin_at_other_sizes(seed, shape):
    a_side, b_sides = S.random_sides(seed, *shape)
    with Handles(a_side, b_sides, host_only=False) as h:
        for kind in KINDS:
            for run, ratio, ori in S.RUNS:
                got = search(h, kind, ratio, ori, False)
                equal(got[:3], R.search_call(a_side, b_sides, kind, ratio, ori)[:3], f"seed {seed} {kind} {run}")
                twin = search(h, kind, ratio, ori, True)
                equal(got[:3], twin[:3], f"seed {seed} {kind} {run} host twin")
                assert got[3][3:5].tolist() == twin[3][3:5].tolist()


@pytest.mark.gpu
def test_device_launch_free_shapes_and_refusals():
    from plvs_amd.keyframe import search_by_bow_kf
    s, where = S.scenario()
    a_side = s["A0"]
    with Handles(a_side, [s["B"][where["no_common_node"]["k"]], s["B"][where["all_invalid"]["k"]], s["empty"]], host_only=False) as h:
        assert h.a.bow_info()["device_bytes"] > 0 and h.a.info()["device_bytes"] == h.a.info()["host_bytes"]
        for kind in KINDS:
            bs, sides = (h.bs, h.b_sides) if kind == R.FRAME else (h.bs[:1] + h.bs[2:], h.b_sides[:1] + h.b_sides[2:])
            # (the kf kind launches for a key frame whose map points are all invalid — its serial side, A0, has valid features — so it is left out there)
            m, d, n, st = search(h, kind, 0.75, 1, False, bs=bs, b_sides=sides)
            assert (m == -1).all() and (n == 0).all() and st.tolist()[:3] == [0, 0, 0], (kind, st)
        out = (np.full((1, len(a_side["desc"])), -5, np.int32), np.full((1, len(a_side["desc"])), -5, np.int32), np.full(1, -5, np.int32),
               np.full(6, -5, np.int32))
        _refused(lambda: search_by_bow_kf(h.a, S.valid_of(a_side), [h.bs[0]], [S.valid_of(h.b_sides[0])], float("nan"), 1, outputs=out))
        with S.key_frame(a_side, host_only=True) as host_only:
            _refused(lambda: search_by_bow_kf(h.a, S.valid_of(a_side), [host_only], [S.valid_of(a_side)], 0.75, 1, outputs=out))
        assert all((o == -5).all() for o in out)
