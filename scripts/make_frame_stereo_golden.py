#!/usr/bin/env python3
"""Golden outputs of the REFERENCE'S OWN Frame::ComputeStereoLineMatches (with LineMatcher::SearchStereoMatchesByKnn and
ComputeDescriptorMatches inside it) on tests/frame_stereo_scenario.py: scripts/ref_wrap/frame_stereo_ref_wrap.cpp — calls only
— is compiled into a temporary directory against oracle/_ref/libmatchers_ref.so (src/Frame.cc, src/LineMatcher.cc unmodified)
with the include flags of oracle/ref/Makefile's matchers target, and this script writes
  tests/golden/frame_stereo_reference.npz          the four output arrays of the reference's run + the inputs digest
  tests/golden/frame_stereo_reference_facts.json   per-branch counts: the restatement's counters on the same run, taken only
                                                   after the restatement has reproduced the reference's floats bit for bit
                                                   and its matcher stage the reference's vMatches / vValidMatches
It asserts ON THE REFERENCE'S RUN that the scenario takes every reachable branch, and times the reference's function on one
core at 100 + 100 lines (profiles/frame_stereo_timing.json, key "cpu_reference").  Dev-time tool: needs the reference tree
and the compiled reference library.  Changes nothing under oracle/."""
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
from scripts.make_frame_rgbd_golden import reference_root, same_bits      # noqa: E402
from tests import frame_stereo_restatement as R                           # noqa: E402
from tests import frame_stereo_scenario as S                              # noqa: E402

REACHED = ("ratio_test", "distance", "octave", "replaced", "equal_not_replaced", "rotation_bins_cut", "vertical_span", "overlap",
           "ll0_small", "lr0_small", "lines_equal", "disparity_below", "disparity_above", "short_3d", "view_angle", "median_cut")
UNREACHABLE = ("flag_matched_right", "octave_pm1")
OUT_KEYS = ("u_right_start", "depth_start", "u_right_end", "depth_end")


def build_wrapper(tmp):
    ref, oref, rdir = reference_root(), os.path.join(ROOT, "oracle", "ref"), os.path.join(ROOT, "oracle", "_ref")
    ld = os.path.join(ref, "Thirdparty", "line_descriptor")
    inc = [os.path.join(oref, "slam_shim"), os.path.join(oref, "cv_full"), os.path.join(oref, "eigen_full"), os.path.join(ref, "include"),
           ref, os.path.join(ref, "include", "CameraModels"), os.path.join(ld, "include"), os.path.join(ld, "include", "line_descriptor"),
           os.path.join(ld, "src"), os.path.join(ref, "Thirdparty", "Sophus"), os.path.join(ROOT, "include"), oref]
    out = os.path.join(tmp, "libframe_stereo_ref.so")
    subprocess.run(["g++", "-O2", "-std=c++14", "-fPIC", "-ffp-contract=off", "-fno-fast-math", "-w", *["-I" + i for i in inc],
                    "-include", os.path.join(oref, "slam_shim", "slam_shim.h"), "-shared",
                    os.path.join(ROOT, "scripts", "ref_wrap", "frame_stereo_ref_wrap.cpp"), "-o", out, "-L" + rdir,
                    "-l:libmatchers_ref.so", "-Wl,-rpath," + rdir], check=True)
    return ctypes.CDLL(out), ctypes.CDLL(os.path.join(rdir, "libmatchers_ref.so"))


def _p(a):
    return np.ascontiguousarray(a).ctypes.data_as(ctypes.c_void_p)


def ref_line_matches(lib, kl, desc, klr, desc_r, sigma2, K4, mbf, max_dist, min_len):
    n = len(kl)
    out = [np.empty(n, np.float32) for _ in range(4)]
    kl, desc, klr, desc_r = (np.ascontiguousarray(a) for a in (kl, desc, klr, desc_r))
    sigma2, K4 = np.ascontiguousarray(sigma2, np.float32), np.ascontiguousarray(K4, np.float32)
    f = ctypes.c_float
    lib.ref_frame_compute_stereo_line_matches(_p(kl), _p(desc), n, _p(klr), _p(desc_r), len(klr), _p(sigma2), len(sigma2), _p(K4),
                                              f(float(mbf)), f(float(max_dist)), f(float(min_len)), *[_p(o) for o in out])
    return out


def ref_matcher(mlib, inp):
    """vMatches / vValidMatches of the reference's SearchStereoMatchesByKnn, through the wrapper oracle/ref builds."""
    kl, klr = inp["keylines"], inp["keylines_right"]
    n, nr = len(kl), len(klr)
    mq, mt, md, mv = np.zeros(nr, np.int32), np.zeros(nr, np.int32), np.zeros(nr, np.float32), np.zeros(nr, np.uint8)
    k = ctypes.c_int()
    mlib.ref_lines_search_stereo_by_knn(_p(inp["desc"]), n, _p(kl["angle"].copy()), _p(kl["octave"].copy()), _p(inp["desc_right"]), nr,
                                        _p(klr["angle"].copy()), _p(klr["octave"].copy()), ctypes.c_float(inp["nn_ratio"]),
                                        int(inp["check_orientation"]), int(inp["descriptor_dist"]), _p(mq), _p(mt), _p(md), _p(mv),
                                        ctypes.byref(k))
    k = k.value
    return [[int(a), int(b), float(c)] for a, b, c in zip(mq[:k], mt[:k], md[:k])], [bool(v) for v in mv[:k]]


def time_reference(lib):
    kl, desc, klr, desc_r = S.random_inputs(100, 100, seed=7)
    us = []
    for k in range(60):
        t0 = time.perf_counter()
        ref_line_matches(lib, kl, desc, klr, desc_r, S.LEVEL_SIGMA2, S.K4, S.MBF, S.LINE_STEREO_MAX_DIST, 0.01)
        if k >= 10:
            us.append((time.perf_counter() - t0) * 1e6)
    return dict(what="Frame::ComputeStereoLineMatches of the reference (src/Frame.cc + src/LineMatcher.cc as oracle/_ref/libmatchers_ref.so "
                     "builds them: -O2, no contraction), one core, 100 + 100 lines (tests/frame_stereo_scenario.random_inputs(100, 100, 7)), "
                     "wall clock per call incl. filling the Frame; median of 50",
                source="scripts/make_frame_stereo_golden.py", us_median=round(float(np.median(us)), 1),
                us_p10=round(float(np.percentile(us, 10)), 1), us_p90=round(float(np.percentile(us, 90)), 1))


def main():
    inp = S.inputs()
    with tempfile.TemporaryDirectory() as tmp:
        lib, mlib = build_wrapper(tmp)
        out = ref_line_matches(lib, inp["keylines"], inp["desc"], inp["keylines_right"], inp["desc_right"], inp["level_sigma2"], inp["K4"],
                               inp["mbf"], inp["line_stereo_max_dist"], inp["min_line_length_3d"])
        ref_m, ref_v = ref_matcher(mlib, inp)
        timing = time_reference(lib)
    # the restatement beside the reference: bit for bit, then its counters are the reference's branch counts
    counters, matcher = {}, {}
    r = R.stereo_line_matches(inp["keylines"], inp["desc"], inp["keylines_right"], inp["desc_right"], *S.args_of(inp), counters=counters,
                              matcher=matcher)
    assert [[q, t, float(d)] for q, t, d in matcher["matches"]] == ref_m and matcher["valid"] == ref_v, \
        "matcher stage: the restatement differs from the reference's vMatches / vValidMatches"
    bad = sum(int((a.view(np.uint32) != b.view(np.uint32)).sum()) for a, b in zip(r[:4], out))
    assert bad == 0, f"the restatement differs from the reference in {bad} floats"
    assert all(same_bits(a, b) for a, b in zip(r[:4], out))
    facts = dict(lines_left=len(inp["keylines"]), lines_right=len(inp["keylines_right"]), matches=len(ref_m),
                 **{k: int(v) for k, v in counters.items()})
    assert facts["stereo"] == int((out[1] > 0).sum()) and all((out[1] > 0) == (out[3] > 0))
    for k in REACHED:
        assert facts[k] >= 1, f"the reference's run does not take the branch {k}"
    for k in UNREACHABLE:
        assert facts[k] == 0, k
    assert facts["stereo"] >= 8, facts
    # the scene's placed cases, read back from the reference's matches
    w = inp["where"]
    holder = {t: q for q, t, _ in ref_m}
    for first, second, t in w["later_closer"]:
        assert holder[t] == second
    for first, second, t in w["equal"] + w["later_farther"]:
        assert holder[t] == first
    for q in w["median_cut"] + w["rotation_cut"]:
        assert out[1][q] == -1
    idx, dist, low = R.knn2_mih(inp["desc"], inp["desc_right"])
    tie = w["mih_tie"]
    q = tie["query"]
    assert dist[q, 0] == dist[q, 1] == 10 and list(idx[q]) == [tie["packed"], tie["spread"]] and tie["spread"] < tie["packed"] \
        and low[q, 0] == tie["spread"], "the tie query does not tell the multi-index-hash order from the lowest index"
    facts["mih_tie"] = dict(query=q, distance=10, first_neighbour_multi_index_hash=int(idx[q, 0]), first_neighbour_lowest_index=int(low[q, 0]),
                            note="equal first and second distances fail the ratio test for any ratio <= 1: the order shows in the k = 2 "
                                 "result and with nn_ratio > 1 (tests/test_frame_stereo.py), not in the reference's outputs")
    facts["unreachable"] = dict(flag_matched_right="every right line occurs once in vMatches (src/Frame.cc:2068)",
                                octave_pm1="the matcher keeps equal octaves only (src/LineMatcher.cc:487 before src/Frame.cc:2078)")
    gdir = os.path.join(ROOT, "tests", "golden")
    np.savez_compressed(os.path.join(gdir, "frame_stereo_reference.npz"), **dict(zip(OUT_KEYS, out)),
                        inputs_digest=np.array(S.inputs_digest(inp)))
    with open(os.path.join(gdir, "frame_stereo_reference_facts.json"), "w") as fh:
        json.dump(dict(what="branch counts of the reference's Frame::ComputeStereoLineMatches on tests/frame_stereo_scenario.py "
                            "(see scripts/make_frame_stereo_golden.py)",
                       inputs=S.inputs_digest(inp), facts=facts), fh, indent=1)
    tpath = os.path.join(ROOT, "profiles", "frame_stereo_timing.json")
    doc = {}
    if os.path.exists(tpath):
        with open(tpath) as fh:
            doc = json.load(fh)
    doc["cpu_reference"] = timing
    with open(tpath, "w") as fh:
        json.dump(doc, fh, indent=1)
    print(facts, timing)


if __name__ == "__main__":
    main()
