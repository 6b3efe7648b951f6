#!/usr/bin/env python3
"""Golden outputs of the REFERENCE'S OWN ORBmatcher::SearchByBoW(pKF1, pKF2, vpMatches12) (src/ORBmatcher.cc:853-997) and
SearchByBoW(pKF, F, vpMapPointMatches) (:300-507) on tests/bow_search_scenario.py.  The two definitions, ORBmatcher::ComputeThreeMaxima
(:2123-2164), ORBmatcher::DescriptorDistance (:2167-2227), the matcher's constants (:57-64) and USE_NEW_HISTOGRAM_FACTOR (:52) are cut
verbatim out of the reference tree into a temporary directory at build time and compiled around
scripts/ref_wrap/bow_search_ref_wrap.cpp with -O2 -ffp-contract=off -fno-fast-math.  No cut text is kept.

What the compiled run hands out: vpMatches12 / vpMapPointMatches after the call, the return value, per serial feature the number of
distances it took (the accessor of the descriptor rows counts them) and the value its own round(rot * factor) returned.  bestDist1,
bestDist2 and the best above the threshold are locals of the compiled text: the golden takes them from tests/bow_search_restatement.py,
only after the restatement reproduced everything observable bit for bit — the crafted boundaries (49 / 50 / 51, the ratio at
equality, the ties) make the match itself depend on them.

Writes
  tests/golden/bow_search_reference.npz          per call (main / degenerate), kind (kf / frame) and run (bow_search_scenario.RUNS): match,
                                                 match_dist, nmatches [K ...], and per serial feature best1, best2, raw_idx, n_dist, raw_bin, cut
  tests/golden/bow_search_reference_facts.json   the input digests, the counters of the placed cases, where they sit
and, with --time, the compiled cuts' time on one core at the measurement's shapes (profiles/bow_search_timing.json, key
"cpu_reference").  Dev-time tool: needs the reference tree.  Changes nothing under oracle/."""
import ctypes
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from scripts.make_frame_rgbd_golden import reference_root      # noqa: E402
from scripts.make_line_fuse_golden import _cpu_model, same     # noqa: E402
from tests import bow_search_restatement as R                  # noqa: E402
from tests import bow_search_scenario as S                     # noqa: E402

_vp, _i, _f = ctypes.c_void_p, ctypes.c_int, ctypes.c_float
SRC = "src/ORBmatcher.cc"
CUTS = {
    "bow_search_cut_define.inc": ((SRC, r"/^#define USE_NEW_HISTOGRAM_FACTOR/"),),
    "bow_search_cut_constants.inc": ((SRC, r"/^    const int ORBmatcher::TH_HIGH = /,/^#endif/"),),
    "bow_search_cut_defs.inc": ((SRC, r"/^    int ORBmatcher::SearchByBoW\(KeyFramePtr&  pKF,Frame &F, vector<MapPointPtr> &vpMapPointMatches\)$/,/^    }/"),
                                (SRC, r"/^    int ORBmatcher::SearchByBoW\(KeyFramePtr& pKF1, KeyFramePtr& pKF2, vector<MapPointPtr> &vpMatches12\)$/,/^    }/")),
    "bow_search_cut_helpers.inc": ((SRC, r"/^    void ORBmatcher::ComputeThreeMaxima\(/,/^    }/"),
                                   (SRC, r"/^#if 0 *$/ { f = 1 } /^} \/\/ namespace PLVS2/ { f = 0 } f { print }")),
}


def _p(a):
    return None if a is None else np.ascontiguousarray(a).ctypes.data_as(_vp)


def flat(side):
    """-> (node_id u32, offset i32, index u32) of a side's vector, in-order."""
    ids = sorted(side["nodes"])
    lens = [len(side["nodes"][k]) for k in ids]
    idx = np.array([i for k in ids for i in side["nodes"][k]], np.uint32)
    return np.array(ids, np.uint32), np.concatenate([[0], np.cumsum(lens)]).astype(np.int32), idx


def build_wrapper(tmp):
    ref = reference_root()
    for name, cuts in CUTS.items():
        with open(os.path.join(tmp, name), "w") as out:
            for path, pattern in cuts:
                text = subprocess.run(["awk", pattern, os.path.join(ref, path)], check=True, capture_output=True, text=True).stdout
                assert text.strip(), f"nothing cut from {path} by {pattern}"
                out.write(text + "\n")
    with open(os.path.join(tmp, "bow_search_cut_defs.inc")) as fh:
        text = fh.read()
        assert text.count("int ORBmatcher::SearchByBoW(") == 2
        assert text.count("if(bestDist1<=TH_LOW)") == 1 and text.count("if(bestDist1<TH_LOW)") == 1
        assert text.count("if(vbMatched2[idx2] || !pMP2)") == 1 and text.count("if(vpMapPointMatches[realIdxF])") == 2
        assert text.count("ComputeThreeMaxima(rotHist,HISTO_LENGTH,ind1,ind2,ind3);") == 2 and text.count("round(rot*factor)") == 3
    with open(os.path.join(tmp, "bow_search_cut_helpers.inc")) as fh:
        text = fh.read()
        assert text.count("int ORBmatcher::DescriptorDistance(") == 2 and text.count("#if 0") == 1, "the two DescriptorDistance bodies and their #if"
    so = os.path.join(tmp, "libbow_search_ref.so")
    subprocess.run(["g++", "-O2", "-std=c++14", "-fPIC", "-ffp-contract=off", "-fno-fast-math", "-w", "-I" + tmp, "-shared",
                    os.path.join(ROOT, "scripts", "ref_wrap", "bow_search_ref_wrap.cpp"), "-o", so], check=True)
    lib = ctypes.CDLL(so)
    side = [_i, _vp, _vp, _vp, _i, _vp, _vp, _vp]
    lib.ref_bow_kf_kf.restype = _i
    lib.ref_bow_kf_kf.argtypes = side + side + [_f, _i, _vp, _vp, _vp]
    lib.ref_bow_kf_frame.restype = _i
    lib.ref_bow_kf_frame.argtypes = side + [_i, _vp, _vp, _i, _vp, _vp, _vp] + [_f, _i, _vp, _vp, _vp]
    assert lib.ref_th_low() == R.TH_LOW and lib.ref_histo_length() == R.HISTO_LENGTH
    return lib


def side_args(side, with_valid=True):
    ids, off, idx = flat(side)
    keep = (np.ascontiguousarray(side["desc"]), np.ascontiguousarray(side["angle"], np.float32), np.ascontiguousarray(side["ref_valid"]), ids, off, idx)
    args = [len(side["desc"]), _p(keep[0]), _p(keep[1])] + ([_p(keep[2])] if with_valid else []) + [len(ids), _p(ids), _p(off), _p(idx)]
    return args, keep


def ref_search(lib, serial, lane, kind, nn_ratio, check_orientation, record=True):
    ns, nl = len(serial["desc"]), len(lane["desc"])
    n_out = nl if kind == R.FRAME else ns
    match = np.full(max(n_out, 1), -9, np.int32)
    n_dist, bin_of = np.zeros(max(ns, 1), np.int32), np.zeros(max(ns, 1), np.int32)
    sa, k1 = side_args(serial)
    la, k2 = side_args(lane, with_valid=kind == R.KF)
    f = lib.ref_bow_kf_kf if kind == R.KF else lib.ref_bow_kf_frame
    n = f(*sa, *la, float(nn_ratio), int(check_orientation), _p(match) if record else None, _p(n_dist) if record else None, _p(bin_of) if record else None)
    return dict(match=match[:n_out], nmatches=n, n_dist=n_dist[:ns], raw_bin=bin_of[:ns])


def compare(ref, rest, name):
    assert same(ref["match"], rest["match"]), f"{name}: match differs at {np.argwhere(ref['match'] != rest['match'])[:8].tolist()}"
    assert ref["nmatches"] == rest["nmatches"] == int((rest["match"] >= 0).sum()), f"{name}: nmatches {ref['nmatches']} / {rest['nmatches']}"
    assert same(ref["n_dist"], rest["n_dist"]), f"{name}: the distances taken differ at {np.argwhere(ref['n_dist'] != rest['n_dist'])[:8].tolist()}"
    assert same(ref["raw_bin"], rest["raw_bin"]), f"{name}: the bins differ at {np.argwhere(ref['raw_bin'] != rest['raw_bin'])[:8].tolist()}"


def run_call(lib, a_side, b_sides, kind, nn_ratio, check_orientation, counts, name):
    out = []
    for k, b in enumerate(b_sides):
        serial, lane = (a_side, b) if kind == R.KF else (b, a_side)
        rest = R.search(serial, lane, kind, nn_ratio, check_orientation, counts)
        compare(ref_search(lib, serial, lane, kind, nn_ratio, check_orientation), rest, f"{name} k={k}")
        out.append(rest)
    return out


def time_reference(lib):
    out = {}
    for key, kind, K, ratio in (("loop_detection", R.KF, 33, 0.9), ("relocalisation", R.FRAME, 10, 0.75)):
        a, bs = S.nominal(K)
        us = []
        for rep in range(7):
            t0 = time.perf_counter()
            for b in bs:
                serial, lane = (a, b) if kind == R.KF else (b, a)
                ref_search(lib, serial, lane, kind, ratio, 1, record=False)
            if rep >= 2:
                us.append((time.perf_counter() - t0) * 1e6)
        out[key] = dict(shape=[K, len(a["desc"]), len(a["nodes"])], us_median=round(float(np.median(us)), 1), us_min=round(float(np.min(us)), 1),
                        us_max=round(float(np.max(us)), 1))
    out["what"] = ("the reference's two ORBmatcher::SearchByBoW overloads as compiled by scripts/make_bow_search_golden.py (-O2, no contraction), one "
                   "call per key frame at tests/bow_search_scenario.nominal(K), one core, wall clock incl. filling the objects (the feature-vector "
                   "std::maps among them); median, min and max of 5 after 2")
    out["machine"] = f"{_cpu_model()}, {os.cpu_count()} logical CPUs (the host that ran this script, not the MI355X host of the GPU figures)"
    out["source"] = "scripts/make_bow_search_golden.py --time"
    return out


def main():
    arrays, facts_counts = {}, {}
    with tempfile.TemporaryDirectory() as tmp:
        lib = build_wrapper(tmp)
        for cname, (a_side, b_sides) in S.calls().items():
            for kind in (R.KF, R.FRAME):
                for run, ratio, ori in S.RUNS:
                    counts = {}
                    per_k = run_call(lib, a_side, b_sides, kind, ratio, ori, counts, f"{cname} {kind} {run}")
                    facts_counts[f"{cname}_{kind}_{run}"] = {k: (v if isinstance(v, list) else int(v)) for k, v in counts.items()}
                    pre = f"{cname}_{kind}_{run}_"
                    arrays[pre + "nmatches"] = np.array([r["nmatches"] for r in per_k], np.int32)
                    for key in ("match", "match_dist", "best1", "best2", "raw_idx", "n_dist", "raw_bin", "cut"):
                        arrays[pre + key] = np.concatenate([np.asarray(r[key]).astype(np.int16) for r in per_k])
        for seed, shape in ((3, (150, 120, 3, 12)), (4, (90, 200, 2, 5))):
            a, bs = S.random_sides(seed, *shape)
            for kind in (R.KF, R.FRAME):
                for run, ratio, ori in S.RUNS:
                    run_call(lib, a, bs, kind, ratio, ori, None, f"random {seed} {kind} {run}")
        timing = time_reference(lib) if "--time" in sys.argv else None
    # ---- the placed cases, on the compiled run (the counters are the restatement's, taken after it reproduced the compiled cuts)
    placed = check_placed(arrays, facts_counts)
    digests = S.digests()
    gdir = os.path.join(ROOT, "tests", "golden")
    np.savez_compressed(os.path.join(gdir, "bow_search_reference.npz"), **arrays)
    _, where = S.scenario()
    with open(os.path.join(gdir, "bow_search_reference_facts.json"), "w") as fh:
        json.dump(dict(what="the reference's two ORBmatcher::SearchByBoW overloads on tests/bow_search_scenario.py: the input digests, the "
                            "restatement's counters of the placed cases (taken only after the restatement reproduced the compiled cuts bit for "
                            "bit), and what the compiled run did at every placed case (see scripts/make_bow_search_golden.py)",
                       digests=digests, runs=[list(r) for r in S.RUNS], counts=facts_counts, placed=placed, where=where), fh, indent=1)
    if timing:
        tpath = os.path.join(ROOT, "profiles", "bow_search_timing.json")
        doc = {}
        if os.path.exists(tpath):
            with open(tpath) as fh:
                doc = json.load(fh)
        doc["cpu_reference"] = timing
        with open(tpath, "w") as fh:
            json.dump(doc, fh, indent=1)
    print(json.dumps(placed)[:3000], timing)


def check_placed(arrays, counts):
    """Every placed case, asserted on the golden arrays (test_bow_search.py asserts the same from the files).  -> what is recorded."""
    sides, where = S.scenario()
    a_side, b_sides = S.calls()["main"]
    placed = {}

    def per_serial(kind, run, k, key):
        """the per-serial-feature array `key` of pair k of the main call"""
        lens = [len(a_side["desc"]) if kind == R.KF else len(b["desc"]) for b in b_sides]
        at = int(np.sum(lens[:k]))
        return arrays[f"main_{kind}_{run}_{key}"][at:at + lens[k]]

    def q(name, kind, run, key, which=0):
        w = where[f"{name}_{kind}"]
        return int(per_serial(kind, run, w["k"], key)[w["queries"][which]])

    for kind in (R.KF, R.FRAME):
        lo, hi = "r075_ori", "r15_plain"
        P = {}
        w = where
        P["single_member_best2"] = q("single_member", kind, lo, "best2")
        assert P["single_member_best2"] == 256 and q("single_member", kind, lo, "raw_idx") == w[f"single_member_{kind}"]["members"][0]
        for name in ("equal_minima", "tie_descending"):
            m = w[f"{name}_{kind}"]["members"]
            first = m[0] if name == "equal_minima" else m[1]
            assert q(name, kind, lo, "best1") == q(name, kind, lo, "best2") == 30
            assert q(name, kind, lo, "raw_idx") == first and q(name, kind, hi, "raw_idx") == first
            P[name] = dict(winner=first, other=[i for i in m if i != first][0], accepted_r075=int(matched(arrays, kind, lo, name, where, a_side, b_sides)),
                           accepted_r15=int(matched(arrays, kind, hi, name, where, a_side, b_sides)))
            assert P[name]["accepted_r075"] == 0 and P[name]["accepted_r15"] == 1
        assert P["tie_descending"]["winner"] > P["tie_descending"]["other"], "the tie's winner is not the higher index"
        m = w[f"second_taken_{kind}"]["members"]
        assert q("second_taken", kind, lo, "raw_idx", 0) == m[0] and q("second_taken", kind, lo, "raw_idx", 1) == m[1]
        assert q("second_taken", kind, lo, "best1", 1) == 27 and q("second_taken", kind, lo, "n_dist", 1) == q("second_taken", kind, lo, "n_dist", 0) - 1
        assert q("all_closed", kind, lo, "best1", 1) == 256 and q("all_closed", kind, lo, "n_dist", 1) == 0 and q("all_closed", kind, lo, "raw_idx", 0) >= 0
        P["thresholds"] = {}
        for bits in (49, 50, 51):
            assert q(f"at_{bits}", kind, lo, "best1") == bits
            P["thresholds"][str(bits)] = int(matched(arrays, kind, lo, f"at_{bits}", where, a_side, b_sides))
        assert P["thresholds"] == ({"49": 1, "50": 0, "51": 0} if kind == R.KF else {"49": 1, "50": 1, "51": 0}), P["thresholds"]
        assert (q("ratio_equal", kind, lo, "best1"), q("ratio_equal", kind, lo, "best2")) == (30, 40)
        P["ratio_equal"] = dict(r075=int(matched(arrays, kind, lo, "ratio_equal", where, a_side, b_sides)),
                                r09=int(matched(arrays, kind, "r09_ori", "ratio_equal", where, a_side, b_sides)))
        assert P["ratio_equal"] == dict(r075=0, r09=1)
        assert q("bin_12", kind, lo, "raw_bin") == 12
        c = counts[f"main_{kind}_{lo}"]
        for key in ("best2_stays_256", "best1_stays_256_all_closed", "equal_minima", "tie_winner_not_lowest_index", "took_behind_a_closed_best",
                    "best1_at_th_low", "ratio_at_equality", "bin_12", "bin_tie_at_cut", "serial_list_of_1", "cut_by_rotation", "multi_pass_jobs"):
            assert c[key] >= 1, f"{kind}: {key} does not occur: {c}"
        assert (c["best1_at_th_low_accepted"] >= 1) == (kind == R.FRAME)
        want = {1, 2, 63, 64, 65} | ({129} if kind == R.KF else set())
        assert want <= set(c["lane_lengths"]), f"{kind}: claimed-side lengths {c['lane_lengths']}"
        P["lane_lengths"] = c["lane_lengths"]
        d = counts[f"degenerate_{kind}_{lo}"]
        assert d["lane_lengths"] == [200] and d["common_nodes"] == 2 and d["accepted"] > 20, d
        nm = arrays[f"main_{kind}_{lo}_nmatches"]
        assert nm[where["no_common_node"]["k"]] == 0 and nm[where["all_invalid"]["k"]] == 0
        P["bin_tie_nmatches"] = int(nm[where["bin_tie"]["k"]])
        assert P["bin_tie_nmatches"] == 7, "3 + 2 + 2 survive, the tied fourth bin is cut"
        P["nmatches"] = [int(x) for x in nm]
        placed[kind] = P
    return placed


def matched(arrays, kind, run, name, where, a_side, b_sides):
    """did the (first) query of a placed case keep its match through the call?"""
    w = where[f"{name}_{kind}"]
    n = len(a_side["desc"])
    row = arrays[f"main_{kind}_{run}_match"][w["k"] * n:(w["k"] + 1) * n]
    if kind == R.KF:
        return row[w["queries"][0]] >= 0
    return bool((row == w["queries"][0]).any())


if __name__ == "__main__":
    main()
