#!/usr/bin/env python3
"""Golden outputs of the REFERENCE'S OWN loop-closing searches — ORBmatcher::SearchByProjection(pKF, Scw, vpPoints, vpMatched, th,
ratioHamming) (src/ORBmatcher.cc:509-615), its overload with vpPointsKFs / vpMatchedKF (:617-730), LineMatcher::SearchByProjection(pKF,
Scw, vpLines, vpMatched, th, ratioHamming) (src/LineMatcher.cc:1767-1909) and its overload with vpLinesKFs / vpMatchedKF (:1913-2037),
as LoopClosing::DetectCommonRegionsFromBoW and FindMatchesByProjection call them — on tests/loop_search_scenario.py.  The four
definitions and the helpers the earlier makers cut (KeyFrame::GetFeaturesInArea, KeyFrame::IsInImage, both PredictScale,
Pinhole::project, the three statements of Sophus' point action, LineProjection::ProjectLineWithCheck, both
KeyFrame::GetLineFeaturesInArea overloads, Geom2DUtils::GetLine2dRepresentation(NoTheta), the distance getters, projectLinear, the
constants and #defines) are cut verbatim out of the reference tree into a temporary directory at build time and compiled around
scripts/ref_wrap/loop_search_ref_wrap.cpp, once per kind, against oracle/ref/eigen_full with -O2 -ffp-contract=off -fno-fast-math.
What each pair did comes from the accessors the compiled text called, and the match from vpMatched / vpMatchedKF after the call.

OUTSIDE THE PIN: Eigen's decomposition of Scw (normalise, toRotationMatrix, matrix -> quaternion) — Eigen is not in the reference
tree, as before.  The wrap's stand-in Sim3f / SE3f hand the scenario's decomposed pose through; Scw.translation() / Scw.scale() and the
line side's Ow = -Rcw.transpose() * tcw (:1770-1773) ARE compiled, and asserted equal to the scenario's tcw and Ow_lines.

Writes
  tests/golden/loop_search_reference.npz          per set (point_ / point_crowd_ / line_ / line_crowd_) and run (tests/loop_search_scenario.RUNS: overload,
                                                  ratio): reached, bestIdx, bestDist, distances taken, projections, levels, the match,
                                                  nmatches + the inputs digests
  tests/golden/loop_search_reference_facts.json   per-branch counts, the placed cases, the overloads compiled
and, with --time, the compiled cuts' time on one core at the measurement's shapes (profiles/loop_search_timing.json, key
"cpu_reference").  Dev-time tool: needs the reference tree.  Changes nothing under oracle/; no cut text is kept."""
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
from scripts.make_line_fuse_golden import CUTS as LINE_CUTS, _cpu_model, _one_of, same      # noqa: E402
from scripts.make_loop_fuse_golden import line_kf_create, point_kf_create      # noqa: E402
from scripts.make_orb_fuse_golden import CUTS as POINT_CUTS    # noqa: E402
from tests import loop_search_restatement as R                 # noqa: E402
from tests import loop_search_scenario as S                    # noqa: E402
from tests import line_fuse_restatement as LR                  # noqa: E402
from tests import orb_fuse_restatement as PR                   # noqa: E402

_vp, _i, _f = ctypes.c_void_p, ctypes.c_int, ctypes.c_float
SEARCH_0 = r"/^    int ORBmatcher::SearchByProjection\(KeyFramePtr& pKF, Sophus::Sim3f &Scw, const vector<MapPointPtr> &vpPoints,$/,/^    }/"
SEARCH_1 = (r"/^    int ORBmatcher::SearchByProjection\(KeyFramePtr& pKF, Sophus::Sim3<float> &Scw, const std::vector<MapPointPtr> &vpPoints, "
            r"const std::vector<KeyFramePtr> &vpPointsKFs,$/,/^    }/")
LINE_SEARCH_0 = r"/^int LineMatcher::SearchByProjection\(KeyFramePtr& pKF, const Sophus::Sim3f& Scw, const vector<MapLinePtr> &vpLines, vector<MapLinePtr> &vpMatched, int th, float ratioHamming\)/,/^}/"
LINE_SEARCH_1 = (r"/^int LineMatcher::SearchByProjection\(KeyFramePtr& pKF, const Sophus::Sim3f& Scw, const std::vector<MapLinePtr> &vpLines, "
                 r"const std::vector<KeyFramePtr> &vpLinesKFs,$/,/^}/")
# :1770-1773 of the first definition alone
LINE_POSE = (r"/^int LineMatcher::SearchByProjection\(KeyFramePtr& pKF, const Sophus::Sim3f& Scw, const vector<MapLinePtr> &vpLines, vector/ { f = 1 } "
             r"f && /Eigen::Matrix3f Rcw = Scw.rotationMatrix\(\);/ { g = 1 } f && g { print } "
             r"f && g && /Eigen::Vector3f Ow = -Rcw.transpose\(\)\*tcw;/ { exit }")
GOT_WORLD_POS, CAMERA_PROJECT, IMAGE_TESTED, GOT_MAX_DISTANCE, GOT_NORMAL, PREDICTED, GOT_DESCRIPTOR = (1 << b for b in range(7))


def _cuts():
    """The SE3 maker's helper cuts, each definition that the wrap compiles under another name in a file of its own."""
    helper = {}
    for name in ("KeyFrame::GetFeaturesInArea", "KeyFrame::IsInImage", "MapPoint::PredictScale", "Pinhole::project"):
        (helper[name.split("::")[1]],) = [c for c in POINT_CUTS["orb_fuse_cut_defs.inc"] if name in c[1]]
    return {"loop_search_cut_so3.inc": POINT_CUTS["orb_fuse_cut_so3.inc"],
            "loop_search_cut_helpers.inc": (helper["GetFeaturesInArea"], helper["project"]),
            "loop_search_cut_isinimage.inc": (helper["IsInImage"],), "loop_search_cut_predict.inc": (helper["PredictScale"],),
            "loop_search_cut_point_defs.inc": (("src/ORBmatcher.cc", SEARCH_0), ("src/ORBmatcher.cc", SEARCH_1)),
            "loop_search_cut_macros.inc": LINE_CUTS["line_fuse_cut_macros.inc"], "loop_search_cut_geom.inc": LINE_CUTS["line_fuse_cut_geom.inc"],
            "loop_search_cut_accessors.inc": LINE_CUTS["line_fuse_cut_accessors.inc"],
            "loop_search_cut_lineproj.inc": LINE_CUTS["line_fuse_cut_lineproj.inc"],
            "loop_search_cut_line_defs.inc": tuple(c for c in LINE_CUTS["line_fuse_cut_defs.inc"] if "::Fuse" not in c[1] and "kChiSquare" not in c[1])
            + (("src/LineMatcher.cc", LINE_SEARCH_0), ("src/LineMatcher.cc", LINE_SEARCH_1)),
            "loop_search_cut_line_pose.inc": (("src/LineMatcher.cc", LINE_POSE),)}


def _p(a):
    return None if a is None else np.ascontiguousarray(a).ctypes.data_as(_vp)


def build_wrapper(tmp):
    ref, oref = reference_root(), os.path.join(ROOT, "oracle", "ref")
    for name, cuts in _cuts().items():
        with open(os.path.join(tmp, name), "w") as out:
            for path, pattern in cuts:
                text = subprocess.run(["awk", pattern, os.path.join(ref, path)], check=True, capture_output=True, text=True).stdout
                assert text.strip(), f"nothing cut from {path} by {pattern}"
                out.write(text + "\n")
    with open(os.path.join(tmp, "loop_search_cut_point_defs.inc")) as fh:
        text = fh.read()
        assert text.count("Sophus::SE3f Tcw = Sophus::SE3f(Scw.rotationMatrix(),Scw.translation()/Scw.scale());") == 2
        assert text.count("if(vpMatched[idx])") == 2 and text.count("if(bestDist<=TH_LOW*ratioHamming)") == 2
        assert text.count("pKF->mpCamera->project(p3Dc)") == 1 and text.count("const float invz = 1/p3Dc(2);") == 1
        assert text.count("vpMatchedKF[bestIdx] = pKFi;") == 1
    with open(os.path.join(tmp, "loop_search_cut_line_pose.inc")) as fh:
        assert len([ln for ln in fh.read().splitlines() if ln.strip()]) == 4, "the line side's decomposition is no longer four statements"
    with open(os.path.join(tmp, "loop_search_cut_line_defs.inc")) as fh:
        text = fh.read()
        assert text.count("if(vpMatched[idx])") == 2 and text.count("if( (bestDist<=TH_LOW*ratioHamming) && (bestIdx>=0) )") == 2
        assert text.count("vpMatchedKF[bestIdx] = pKFi;") == 1 and text.count("proj.ProjectLineWithCheck(pML, *pKF, frameTransforms)") == 2
    libs, names = {}, {}
    for kind in ("POINTS", "LINES"):
        so = os.path.join(tmp, f"libloop_search_{kind.lower()}_ref.so")
        subprocess.run(["g++", "-O2", "-std=c++14", "-fPIC", "-ffp-contract=off", "-fno-fast-math", "-w", "-DLOOP_SEARCH_WRAP_" + kind,
                        "-I" + os.path.join(oref, "eigen_full"), "-I" + tmp, "-shared",
                        os.path.join(ROOT, "scripts", "ref_wrap", "loop_search_ref_wrap.cpp"), "-o", so], check=True)
        undefined = subprocess.run(["nm", "-D", "--undefined-only", so], check=True, capture_output=True, text=True).stdout.split()
        names[kind] = {u.split("@")[0] for u in undefined}
        libs[kind] = ctypes.CDLL(so)
    lib, ll = libs["POINTS"], libs["LINES"]
    overloads = dict(point_log="std::log(float)" if _one_of(names["POINTS"], "logf", "log", "MapPoint::PredictScale") else "::log(double)",
                     line_log="std::log(float)" if _one_of(names["LINES"], "logf", "log", "MapLine::PredictScale") else "::log(double)",
                     atan2="atan2f" if _one_of(names["LINES"], "atan2f", "atan2", "GetLine2dRepresentation") else "atan2")
    ll.ref_line_kf_create.restype = _vp
    ll.ref_line_kf_create.argtypes = [_i] + [_vp] * 6 + [_f, _vp, _f, _vp, _vp, _f, _i, _vp, _vp, _f]
    ll.ref_line_kf_destroy.argtypes = [_vp]
    ll.ref_line_kf_destroy.restype = None
    ll.ref_line_pose.argtypes = [_vp, _vp, _vp]
    ll.ref_line_pose.restype = None
    ll.ref_line_search.restype = _i
    ll.ref_line_search.argtypes = [_vp, _i, _i] + [_vp] * 7 + [_i, _f, _vp, _vp, _vp]
    ll.ref_line_search_plain.restype = _i
    ll.ref_line_search_plain.argtypes = [_vp, _i, _i] + [_vp] * 6 + [_i, _f]
    assert ll.ref_th_low() == R.LINE_TH_LOW
    lib.ref_kf_create.restype = _vp
    lib.ref_kf_create.argtypes = [_i] + [_vp] * 6 + [_f, _f, _vp, _f, _vp, _vp, _f, _vp, _vp, _i, _vp, _vp, _f]
    lib.ref_kf_destroy.argtypes = [_vp]
    lib.ref_kf_destroy.restype = None
    lib.ref_search.restype = _i
    lib.ref_search.argtypes = [_vp, _i, _i] + [_vp] * 7 + [_i, _f, _vp, _vp, _vp, _vp]
    lib.ref_search_plain.restype = _i
    lib.ref_search_plain.argtypes = [_vp, _i, _i] + [_vp] * 6 + [_i, _f]
    assert lib.ref_th_low() == R.POINT_TH_LOW
    return lib, ll, overloads


def ref_point_search(lib, inp, projection, ratio):
    """The reference's SearchByProjection, one call per key frame -> the restatement's fields as the accessors record them."""
    pts, K = inp["points"], len(inp["kfs"])
    M = len(pts["min_dist"])
    th = int(inp["th"])
    assert th == inp["th"], "the reference's th is an int"
    o = dict(reached=np.zeros((K, M), np.uint8), match_idx=np.full((K, M), -1, np.int32), raw_best_dist=np.full((K, M), 256, np.int32),
             n_dist=np.zeros((K, M), np.int32), level=np.full((K, M), -1, np.int32), u=np.zeros((K, M), np.float32),
             v=np.zeros((K, M), np.float32), nmatches=np.zeros(K, np.int32))
    T = R.cut_of(R.POINT_TH_LOW, ratio)
    for k, kf in enumerate(inp["kfs"]):
        h, keep = point_kf_create(lib, kf)
        rec, uv, band, tcw = np.zeros((M, 5), np.int32), np.zeros((M, 2), np.float32), np.zeros(M, np.int32), np.zeros(3, np.float32)
        sk = None if inp["skip"] is None else np.ascontiguousarray(inp["skip"][k])
        occ = None if inp["occupied"] is None or inp["occupied"][k] is None else np.ascontiguousarray(inp["occupied"][k], np.uint8)
        o["nmatches"][k] = lib.ref_search(h, projection, M, _p(pts["pos"]), _p(pts["normal"]), _p(pts["min_dist"]), _p(pts["max_dist"]),
                                          _p(pts["desc"]), _p(sk), _p(occ), th, float(ratio), _p(rec), _p(uv), _p(band), _p(tcw))
        lib.ref_kf_destroy(h)
        assert same(tcw, np.asarray(kf["tcw"], np.float32)), f"key frame {k}: the compiled Scw.translation() / Scw.scale() is not the scenario's tcw"
        for i in range(M):
            fl, nd, md, lv, match = (int(c) for c in rec[i])
            assert bool(fl & CAMERA_PROJECT) == (projection == R.CAMERA and bool(fl & IMAGE_TESTED)), "the overload's own projection"
            if not fl & GOT_WORLD_POS:
                r = PR.SKIPPED
            elif not fl & IMAGE_TESTED:
                r = PR.BEHIND
            elif not fl & GOT_MAX_DISTANCE:
                r = PR.OUTSIDE
            elif not fl & GOT_NORMAL:
                assert band[i] in (1, 2), "stopped at the band, and neither comparison of :560 holds"
                r = PR.TOO_NEAR if band[i] == 1 else PR.TOO_FAR
            elif not fl & PREDICTED:
                r = PR.VIEW_ANGLE
            elif not fl & GOT_DESCRIPTOR:
                r = PR.EMPTY_WINDOW
            elif match >= 0:
                assert md <= T and nd >= 1
                r = PR.CANDIDATE
            else:
                assert md > T
                r = None           # bestDist above the cut, or 256: whether anybody passed the band (NO_CANDIDATE) is not the reference's
                                   # to tell when every banded member was claimed — the restatement, compared below, tells
            o["reached"][k, i] = 255 if r is None else r
            o["n_dist"][k, i], o["level"][k, i], o["match_idx"][k, i] = nd, lv, match
            if fl & IMAGE_TESTED:
                o["u"][k, i], o["v"][k, i] = uv[i]
            if nd:
                o["raw_best_dist"][k, i] = md
        assert o["nmatches"][k] == int((o["match_idx"][k] >= 0).sum())
    return o


def compare_points(ref, rest, name):
    open_ = ref["reached"] == 255
    assert np.isin(rest["reached"][open_], (PR.NO_CANDIDATE, PR.ABOVE_TH_LOW)).all(), name
    # NO_CANDIDATE with distances taken, or ABOVE_TH_LOW with none taken and nobody claimed, would contradict the compiled run
    assert not ((rest["reached"] == PR.NO_CANDIDATE) & (ref["n_dist"] > 0)).any(), name
    assert same(np.where(open_, rest["reached"], ref["reached"]), rest["reached"]), f"{name}: reached differs at {np.argwhere(np.where(open_, rest['reached'], ref['reached']) != rest['reached'])[:8]}"
    for k in ("n_dist", "raw_best_dist", "u", "v", "level", "match_idx", "nmatches"):
        assert same(ref[k], rest[k]), f"{name}: {k} differs at {np.argwhere(ref[k] != rest[k])[:8]}"
    assert same(np.where(ref["match_idx"] >= 0, ref["raw_best_dist"], -1), rest["match_dist"]), f"{name}: the match's distance differs"
    out = dict(ref)
    out["reached"] = rest["reached"].copy()
    out["raw_best_idx"] = rest["raw_best_idx"].copy()    # bestIdx of a pair above the cut is not observable in the compiled run
    assert same(np.where(ref["match_idx"] >= 0, out["raw_best_idx"], -1), ref["match_idx"])
    return out


def ref_line_search(lib, inp, overload, ratio):
    GOT_END_POINTS, GOT_MAX_DISTANCE_L, GOT_NORMAL_L, PREDICTED_L, GOT_DESCRIPTOR_L = (1 << b for b in range(5))
    ln, K = inp["lines"], len(inp["kfs"])
    M = len(ln["max_dist"])
    th = int(inp["th"])
    assert th == inp["th"], "the reference's th is an int"
    T = R.cut_of(R.LINE_TH_LOW, ratio)
    o = dict(reached=np.zeros((K, M), np.uint8), match_idx=np.full((K, M), -1, np.int32), raw_best_dist=np.full((K, M), 256, np.int32),
             n_dist=np.zeros((K, M), np.int32), level=np.full((K, M), -1, np.int32), proj=np.zeros((K, M, 6), np.float32),
             n_proj=np.zeros((K, M), np.int32), nmatches=np.zeros(K, np.int32))
    for k, kf in enumerate(inp["kfs"]):
        h, keep = line_kf_create(lib, kf)
        tcw, ow = np.zeros(3, np.float32), np.zeros(3, np.float32)
        lib.ref_line_pose(h, _p(tcw), _p(ow))
        assert same(tcw, np.asarray(kf["tcw"], np.float32)), f"key frame {k}: the compiled Scw.translation() / scale is not the scenario's tcw"
        assert same(ow, np.asarray(kf["Ow_lines"], np.float32)), f"key frame {k}: the compiled -Rcw.transpose() * tcw is not the scenario's Ow_lines"
        rec, proj, stop = np.zeros((M, 6), np.int32), np.zeros((M, 6), np.float32), np.zeros(M, np.int32)
        sk = None if inp["skip"] is None else np.ascontiguousarray(inp["skip"][k])
        occ = None if inp["occupied"] is None or inp["occupied"][k] is None else np.ascontiguousarray(inp["occupied"][k], np.uint8)
        o["nmatches"][k] = lib.ref_line_search(h, overload, M, _p(ln["start"]), _p(ln["end"]), _p(ln["normal"]), _p(ln["max_dist"]), _p(ln["desc"]),
                                               _p(sk), _p(occ), th, float(ratio), _p(rec), _p(proj), _p(stop))
        lib.ref_line_kf_destroy(h)
        for i in range(M):
            fl, npj, nd, md, lv, match = (int(c) for c in rec[i])
            if not fl & GOT_END_POINTS:
                r = LR.SKIPPED
            elif npj == 0:
                r = LR.MIDDLE_BEHIND
            elif not fl & GOT_MAX_DISTANCE_L:
                r = LR.MIDDLE_OUTSIDE
            elif not fl & GOT_NORMAL_L:
                r = {1: LR.TOO_NEAR, 2: LR.TOO_FAR, 3: LR.END_BEHIND, 4: LR.END_OUTSIDE}[int(stop[i])]
            elif not fl & PREDICTED_L:
                r = LR.VIEW_ANGLE
            elif not fl & GOT_DESCRIPTOR_L:
                r = LR.EMPTY_WINDOW
            elif match >= 0:
                assert md <= T and nd >= 1
                r = LR.CANDIDATE
            else:
                assert md > T
                r = 255            # NO_CANDIDATE or ABOVE_TH_LOW: the restatement, compared below, tells (see ref_point_search)
            o["reached"][k, i], o["n_dist"][k, i], o["level"][k, i], o["n_proj"][k, i], o["match_idx"][k, i] = r, nd, lv, min(npj, 3), match
            o["proj"][k, i] = proj[i]
            if nd:
                o["raw_best_dist"][k, i] = md
        assert o["nmatches"][k] == int((o["match_idx"][k] >= 0).sum())
    return o


def compare_lines(ref, rest, name):
    open_ = ref["reached"] == 255
    assert np.isin(rest["reached"][open_], (LR.NO_CANDIDATE, LR.ABOVE_TH_LOW)).all(), name
    assert not ((rest["reached"] == LR.NO_CANDIDATE) & (ref["n_dist"] > 0)).any(), name
    merged = np.where(open_, rest["reached"], ref["reached"])
    assert same(merged, rest["reached"]), f"{name}: reached differs at {np.argwhere(merged != rest['reached'])[:8].tolist()}"
    for k in ("n_dist", "raw_best_dist", "level", "n_proj", "proj", "match_idx", "nmatches"):
        assert same(ref[k], rest[k]), f"{name}: {k} differs at {np.argwhere(ref[k] != rest[k])[:8].tolist()}"
    assert same(np.where(ref["match_idx"] >= 0, ref["raw_best_dist"], -1), rest["match_dist"]), f"{name}: the match's distance differs"
    out = dict(ref)
    out["reached"] = rest["reached"].copy()
    out["raw_best_idx"] = rest["raw_best_idx"].copy()
    return out


def time_reference(lib, ll):
    """One core, the measurement's shapes: the K calls of one overload back to back, as the verification loop makes them."""
    out = {}
    for K in (1, 5):
        inp = S.nominal_point_inputs(K)
        pts = inp["points"]
        M = len(pts["min_dist"])
        args = [_p(pts[k]) for k in ("pos", "normal", "min_dist", "max_dist", "desc")]
        us = []
        for rep in range(7):
            t0 = time.perf_counter()
            for k, kf in enumerate(inp["kfs"]):
                h, keep = point_kf_create(lib, kf)
                lib.ref_search_plain(h, R.CAMERA, M, *args, _p(np.ascontiguousarray(inp["skip"][k])), 3, 1.5)
                lib.ref_kf_destroy(h)
            if rep >= 2:
                us.append((time.perf_counter() - t0) * 1e6)
        out[f"points_K{K}"] = dict(shape=[K, M, len(inp["kfs"][0]["x"])], us_median=round(float(np.median(us)), 1),
                                   us_min=round(float(np.min(us)), 1), us_max=round(float(np.max(us)), 1))
        inp = S.nominal_line_inputs(K)
        it = inp["lines"]
        M = len(it["max_dist"])
        args = [_p(it[k]) for k in ("start", "end", "normal", "max_dist", "desc")]
        us = []
        for rep in range(7):
            t0 = time.perf_counter()
            for k, kf in enumerate(inp["kfs"]):
                h, keep = line_kf_create(ll, kf)
                ll.ref_line_search_plain(h, 0, M, *args, _p(np.ascontiguousarray(inp["skip"][k])), 3, 1.5)
                ll.ref_line_kf_destroy(h)
            if rep >= 2:
                us.append((time.perf_counter() - t0) * 1e6)
        out[f"lines_K{K}"] = dict(shape=[K, M, len(inp["kfs"][0]["kl"])], us_median=round(float(np.median(us)), 1),
                                  us_min=round(float(np.min(us)), 1), us_max=round(float(np.max(us)), 1))
    out["what"] = ("the reference's ORBmatcher:: and LineMatcher::SearchByProjection(pKF, Scw, vp, vpMatched, th 3, ratio 1.5) as compiled by "
                   "scripts/make_loop_search_golden.py (-O2, no contraction), one call per key frame at "
                   "tests/loop_search_scenario.nominal_point_inputs(K) / nominal_line_inputs(K), one core, wall clock incl. filling the objects and the grid; median, "
                   "min and max of 5 after 2")
    out["machine"] = f"{_cpu_model()}, {os.cpu_count()} logical CPUs (the host that ran this script, not the MI355X host of the GPU figures)"
    out["source"] = "scripts/make_loop_search_golden.py --time"
    return out


def main():
    arrays, counts, digests = {}, {}, {}
    with tempfile.TemporaryDirectory() as tmp:
        lib, ll, overloads = build_wrapper(tmp)
        pd, ld, ad = overloads["point_log"] != "std::log(float)", overloads["line_log"] != "std::log(float)", overloads["atan2"] != "atan2f"
        sets = dict(point=S.point_inputs(), point_crowd=S.crowd_point_inputs())
        refs = {}
        for sname, inp in sets.items():
            digests[sname + "_inputs"] = S.digest(inp)
            for run, projection, ratio in S.RUNS:
                c = {}
                rest = R.point_search(inp["kfs"], inp["points"], inp["skip"], inp["occupied"], inp["th"], ratio, projection, c, pd)
                refs[sname, run] = compare_points(ref_point_search(lib, inp, projection, ratio), rest, f"{sname} {run}")
                counts[f"{sname}_{run}"] = c
                arrays.update({f"{sname}_{run}_{k}": v for k, v in refs[sname, run].items()})
        for seed in (3, 4):
            rnd = S.random_point_inputs(3, 150, 200, seed=seed)
            for run, projection, ratio in S.RUNS:
                compare_points(ref_point_search(lib, rnd, projection, ratio),
                               R.point_search(rnd["kfs"], rnd["points"], rnd["skip"], rnd["occupied"], rnd["th"], ratio, projection, None, pd),
                               f"random {seed} {run}")
        lsets = dict(line=S.line_inputs(), line_crowd=S.crowd_line_inputs())
        for sname, inp in lsets.items():
            digests[sname + "_inputs"] = S.digest(inp)
            for run, overload, ratio in S.LINE_RUNS:
                c = {}
                rest = R.line_search(inp["kfs"], inp["lines"], inp["skip"], inp["occupied"], inp["th"], ratio, c, ld, ad)
                refs[sname, run] = compare_lines(ref_line_search(ll, inp, overload, ratio), rest, f"{sname} {run}")
                counts[f"{sname}_{run}"] = c
                arrays.update({f"{sname}_{run}_{k}": v for k, v in refs[sname, run].items()})
        lamb = {}
        for rnd in (S.random_line_inputs(3, 120, 150, seed=3), dict(S.LF.ambiguous_line_inputs(), occupied=None)):
            for run, overload, ratio in S.LINE_RUNS:
                compare_lines(ref_line_search(ll, rnd, overload, ratio),
                              R.line_search(rnd["kfs"], rnd["lines"], rnd["skip"], rnd["occupied"], rnd["th"], ratio, lamb, ld, ad), f"random lines {run}")
        assert lamb["ambiguous_level"] >= 1 and lamb["ambiguous_theta"] >= 1
        timing = time_reference(lib, ll) if "--time" in sys.argv else None
    # ---- the conditions on the scenario, on the compiled run
    inp, w = sets["point"], sets["point"]["where"]
    cam, inv = refs["point", "camera_r15"], refs["point", "invz_r10"]
    for run in ("camera_r15", "invz_r10"):
        c = counts["point_" + run]
        for k in PR.REACHED:
            assert c[k] >= 1, f"{run}: the reference's point run does not take {k}: {c}"
        for k in ("took_behind_a_claimed_best", "all_banded_claimed", "tie_winner_not_lowest_index", "occupied_would_have_won", "dist_at_cut",
                  "dist_at_cut_plus_1"):
            assert c[k] >= 1, f"{run}: {k} does not occur: {c}"
    at = lambda ref, name, f="reached": int(ref[f][0, w[name][0]])
    for ref in (cam, inv):
        a, b = w["second_best_members"]
        assert at(ref, "second_best_first", "match_idx") == a and at(ref, "second_best", "match_idx") == b
        assert at(ref, "all_claimed_first", "match_idx") == w["all_claimed_member"][0]
        assert at(ref, "all_claimed") == PR.ABOVE_TH_LOW and at(ref, "all_claimed", "raw_best_dist") == 256 and at(ref, "all_claimed", "n_dist") == 0
        e, f = w["occupied_members"]
        assert at(ref, "occupied_wins", "match_idx") == f
        ja, jb = w["tie_indices"]
        assert ja > jb and at(ref, "tie", "match_idx") == ja, "the tie's winner is not the higher index"
        for bits in (50, 51, 75, 76):
            assert at(ref, f"at_{bits}", "raw_best_dist") == bits
    assert [at(cam, f"at_{b}") for b in (50, 51, 75, 76)] == [PR.CANDIDATE, PR.CANDIDATE, PR.CANDIDATE, PR.ABOVE_TH_LOW]
    assert [at(inv, f"at_{b}") for b in (50, 51, 75, 76)] == [PR.CANDIDATE, PR.ABOVE_TH_LOW, PR.ABOVE_TH_LOW, PR.ABOVE_TH_LOW]
    i = w["project_bit"][0]
    ua, ub = cam["u"][0, i], inv["u"][0, i]
    assert ua != ub and abs(int(ua.view(np.int32)) - int(ub.view(np.int32))) == 1, "the two projections do not differ in the last bit of u"
    assert {at(cam, "project_bit"), at(inv, "project_bit")} == {PR.CANDIDATE, PR.EMPTY_WINDOW}, "the last bit does not change the result"
    # the crowd: the last two of the same-descriptor points find the first LIST_LEN members claimed
    cw = sets["point_crowd"]["where"]
    for ref in (refs["point_crowd", "camera_r15"], refs["point_crowd", "invz_r10"]):
        got = [int(ref["match_idx"][0, i]) for i in cw["same_descriptor_points"]]
        assert sorted(got) == sorted(cw["same_descriptor_members"]) and len(got) == R.LIST_LEN + 2, got
    for run in ("camera_r15", "invz_r10"):
        assert counts["point_crowd_" + run]["windows_over_list_len"] >= R.LIST_LEN + 2
    # ---- lines: the same conditions on the fourth key frame of the line set
    lw = lsets["line"]["where"]
    l15, l10 = refs["line", "kf0_r15"], refs["line", "kf1_r10"]
    for run in ("kf0_r15", "kf1_r10"):
        c = counts["line_" + run]
        for k in LR.REACHED:
            assert (c[k] >= 1) != (k == "degenerate"), f"{run}: the reference's line run takes {k} {c[k]} times"
        for k in ("took_behind_a_claimed_best", "all_banded_claimed", "tie_winner_not_lowest_index", "occupied_would_have_won", "dist_at_cut",
                  "dist_at_cut_plus_1"):
            assert c[k] >= 1, f"{run}: {k} does not occur: {c}"
    lat = lambda ref, name, f="reached", k=3: int(ref[f][k, lw[name][0]])
    for ref in (l15, l10):
        a, b = lw["second_best_members"]
        assert lat(ref, "second_best_first", "match_idx") == a and lat(ref, "second_best", "match_idx") == b
        assert lat(ref, "all_claimed_first", "match_idx") == lw["all_claimed_member"][0]
        assert lat(ref, "all_claimed") == LR.ABOVE_TH_LOW and lat(ref, "all_claimed", "raw_best_dist") == 256 and lat(ref, "all_claimed", "n_dist") == 0
        assert lat(ref, "occupied_wins", "match_idx") == lw["occupied_members"][1]
        ja, jb = lw["tie_indices"]
        assert ja > jb and lat(ref, "split_plus_tie", "match_idx", 0) == ja, "the tie's winner is not the higher index"
        for bits in (60, 61, 90, 91):
            assert lat(ref, f"at_{bits}", "raw_best_dist") == bits
    assert [lat(l15, f"at_{b}") for b in (60, 61, 90, 91)] == [LR.CANDIDATE, LR.CANDIDATE, LR.CANDIDATE, LR.ABOVE_TH_LOW]
    assert [lat(l10, f"at_{b}") for b in (60, 61, 90, 91)] == [LR.CANDIDATE, LR.ABOVE_TH_LOW, LR.ABOVE_TH_LOW, LR.ABOVE_TH_LOW]
    lcw = lsets["line_crowd"]["where"]
    for ref in (refs["line_crowd", "kf0_r15"], refs["line_crowd", "kf1_r10"]):
        got = [int(ref["match_idx"][1, i]) for i in lcw["same_descriptor_lines"]]
        assert sorted(got) == sorted(lcw["same_descriptor_members"]) and len(got) == R.LIST_LEN + 2, got
    for run in ("kf0_r15", "kf1_r10"):
        assert counts["line_crowd_" + run]["windows_over_list_len"] >= R.LIST_LEN + 2
    for c in counts.values():
        c["cases"] = {k: [int(x) for x in v] for k, v in c["cases"].items()}
    facts = dict(counts=counts, overloads=overloads, double_overloads=dict(point_log=int(pd), line_log=int(ld), atan2=int(ad)),
                 runs=[list(r) for r in S.RUNS], line_runs=[list(r) for r in S.LINE_RUNS],
                 ambiguous_counts=dict(line_level=lamb["ambiguous_level"], line_theta=lamb["ambiguous_theta"]),
                 line_where={k: [int(i) for i in v] for k, v in lw.items()}, line_crowd_where={k: [int(i) for i in v] for k, v in lcw.items()},
                 list_len=R.LIST_LEN, nmatches={f"{s}_{r}": [int(n) for n in v["nmatches"]] for (s, r), v in refs.items()},
                 project_bit=dict(u_camera=float(ua), u_invz=float(ub), reached_camera=at(cam, "project_bit"), reached_invz=at(inv, "project_bit")),
                 point_where={k: [int(i) for i in v] for k, v in w.items()}, point_crowd_where={k: [int(i) for i in v] for k, v in cw.items()})
    gdir = os.path.join(ROOT, "tests", "golden")
    np.savez_compressed(os.path.join(gdir, "loop_search_reference.npz"), **arrays, **{k + "_digest": np.array(v) for k, v in digests.items()})
    with open(os.path.join(gdir, "loop_search_reference_facts.json"), "w") as fh:
        json.dump(dict(what="branch counts of the reference's four loop-closing SearchByProjection overloads (ORBmatcher's and LineMatcher's) on "
                            "tests/loop_search_scenario.py (the restatement's counters, taken only after the restatement reproduced the "
                            "compiled cuts bit for bit), the `log` and `atan2` overloads they were compiled with and the placed cases (see "
                            "scripts/make_loop_search_golden.py); Eigen's decomposition of Scw is outside the pin", digests=digests, facts=facts),
                  fh, indent=1)
    if timing:
        tpath = os.path.join(ROOT, "profiles", "loop_search_timing.json")
        doc = {}
        if os.path.exists(tpath):
            with open(tpath) as fh:
                doc = json.load(fh)
        doc["cpu_reference"] = timing
        with open(tpath, "w") as fh:
            json.dump(doc, fh, indent=1)
    print(json.dumps(facts)[:1500], timing)


if __name__ == "__main__":
    main()
