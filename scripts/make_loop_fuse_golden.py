#!/usr/bin/env python3
"""Golden outputs of the REFERENCE'S OWN Sim3 Fuse overloads — ORBmatcher::Fuse(pKF, Scw, vpPoints, th, vpReplacePoint)
(src/ORBmatcher.cc:1437-1553) and LineMatcher::Fuse(pKF, Scw, vpLines, th, vpReplaceLine) (src/LineMatcher.cc:2321-2561), as the two
overloads of LoopClosing::SearchAndFuse call them — on tests/loop_fuse_scenario.py.  The two definitions and the helpers the SE3
makers cut (KeyFrame::GetFeaturesInArea, KeyFrame::IsInImage, both PredictScale, Pinhole::project, the three statements of Sophus'
point action, LineProjection::ProjectLineWithCheck, both KeyFrame::GetLineFeaturesInArea overloads,
Geom2DUtils::GetLine2dRepresentation(NoTheta), the distance getters, projectLinear, the constants and #defines) are cut verbatim out
of the reference tree into a temporary directory at build time and compiled around scripts/ref_wrap/loop_fuse_ref_wrap.cpp, once
per kind, against oracle/ref/eigen_full with -O2 -ffp-contract=off -fno-fast-math.  What each pair did comes from the accessors the
compiled text called.

OUTSIDE THE PIN: Eigen's decomposition of Scw (normalise, toRotationMatrix, matrix -> quaternion) — Eigen is not in the reference
tree, as OpenCV's primitives are not elsewhere.  The wrap's stand-in Sim3f / SE3f hand the scenario's decomposed pose through;
Scw.translation() / Scw.scale() and the line side's Ow = -Rcw.transpose() * tcw ARE compiled, and asserted equal to the scenario's
tcw and Ow_lines.

Writes
  tests/golden/loop_fuse_reference.npz          per kind (point_ / line_, and their crowd_ sets): reached, bestIdx, bestDist,
                                                distances taken, projections, levels + the inputs digests
  tests/golden/loop_fuse_reference_facts.json   per-branch counts, the overloads compiled, the #defines, the placed cases
and, with --time, the compiled cuts' time on one core at the measurement's loop shape (profiles/loop_fuse_timing.json, key
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
from scripts.make_orb_fuse_golden import CUTS as POINT_CUTS    # noqa: E402
from tests import line_fuse_restatement as LR                  # noqa: E402
from tests import loop_fuse_restatement as R                   # noqa: E402
from tests import loop_fuse_scenario as S                      # noqa: E402
from tests import orb_fuse_restatement as PR                   # noqa: E402

_vp, _i, _f = ctypes.c_void_p, ctypes.c_int, ctypes.c_float
POINT_FUSE = r"/^    int ORBmatcher::Fuse\(KeyFramePtr& pKF, Sophus::Sim3f &Scw, const vector<MapPointPtr> &vpPoints, float th, vector<MapPointPtr> &vpReplacePoint\)/,/^    }/"
LINE_FUSE = r"/^int LineMatcher::Fuse\(KeyFramePtr& pKF, const Sophus::Sim3f& Scw, const std::vector<MapLinePtr> &vpLines, const float th, vector<MapLinePtr> &vpReplaceLine\)/,/^}/"
# :2324-2327 of that definition alone
LINE_POSE = (r"/^int LineMatcher::Fuse\(KeyFramePtr& pKF, const Sophus::Sim3f& Scw/ { f = 1 } "
             r"f && /Eigen::Matrix3f Rcw = Scw.rotationMatrix\(\);/ { g = 1 } f && g { print } "
             r"f && g && /Eigen::Vector3f Ow = -Rcw.transpose\(\)\*tcw;/ { exit }")


def _cuts():
    """The SE3 makers' cuts with the two Fuse definitions swapped for the Sim3 ones, under this maker's file names."""
    is_fuse = lambda pat: "::Fuse" in pat
    point_defs = ((("src/ORBmatcher.cc", POINT_FUSE),) + tuple(c for c in POINT_CUTS["orb_fuse_cut_defs.inc"] if not is_fuse(c[1])))
    line_defs = tuple(c for c in LINE_CUTS["line_fuse_cut_defs.inc"] if not is_fuse(c[1])) + (("src/LineMatcher.cc", LINE_FUSE),)
    assert len(point_defs) == len(POINT_CUTS["orb_fuse_cut_defs.inc"]) and len(line_defs) == len(LINE_CUTS["line_fuse_cut_defs.inc"])
    return {"loop_fuse_cut_point_defs.inc": point_defs, "loop_fuse_cut_so3.inc": POINT_CUTS["orb_fuse_cut_so3.inc"],
            "loop_fuse_cut_macros.inc": LINE_CUTS["line_fuse_cut_macros.inc"], "loop_fuse_cut_geom.inc": LINE_CUTS["line_fuse_cut_geom.inc"],
            "loop_fuse_cut_accessors.inc": LINE_CUTS["line_fuse_cut_accessors.inc"],
            "loop_fuse_cut_lineproj.inc": LINE_CUTS["line_fuse_cut_lineproj.inc"], "loop_fuse_cut_line_defs.inc": line_defs,
            "loop_fuse_cut_line_pose.inc": (("src/LineMatcher.cc", LINE_POSE),)}


def _p(a):
    return None if a is None else np.ascontiguousarray(a).ctypes.data_as(_vp)


def build_wrappers(tmp):
    ref, oref = reference_root(), os.path.join(ROOT, "oracle", "ref")
    for name, cuts in _cuts().items():
        with open(os.path.join(tmp, name), "w") as out:
            for path, pattern in cuts:
                text = subprocess.run(["awk", pattern, os.path.join(ref, path)], check=True, capture_output=True, text=True).stdout
                assert text.strip(), f"nothing cut from {path} by {pattern}"
                out.write(text + "\n")
    with open(os.path.join(tmp, "loop_fuse_cut_line_pose.inc")) as fh:
        assert len([ln for ln in fh.read().splitlines() if ln.strip()]) == 4, "the line side's decomposition is no longer four statements"
    with open(os.path.join(tmp, "loop_fuse_cut_point_defs.inc")) as fh:
        text = fh.read()
        assert "Sophus::SE3f Tcw = Sophus::SE3f(Scw.rotationMatrix(),Scw.translation()/Scw.scale());" in text
        assert "Eigen::Vector3f Ow = Tcw.inverse().translation();" in text and "GetMapPointsUnordered()" in text
    libs, names = {}, {}
    for kind in ("POINTS", "LINES"):
        so = os.path.join(tmp, f"libloop_fuse_{kind.lower()}_ref.so")
        subprocess.run(["g++", "-O2", "-std=c++14", "-fPIC", "-ffp-contract=off", "-fno-fast-math", "-w", "-DLOOP_WRAP_" + kind,
                        "-I" + os.path.join(oref, "eigen_full"), "-I" + tmp, "-shared",
                        os.path.join(ROOT, "scripts", "ref_wrap", "loop_fuse_ref_wrap.cpp"), "-o", so], check=True)
        undefined = subprocess.run(["nm", "-D", "--undefined-only", so], check=True, capture_output=True, text=True).stdout.split()
        names[kind] = {u.split("@")[0] for u in undefined}
        libs[kind] = ctypes.CDLL(so)
    pl, ll = libs["POINTS"], libs["LINES"]
    overloads = dict(point_log="std::log(float)" if _one_of(names["POINTS"], "logf", "log", "MapPoint::PredictScale") else "::log(double)",
                     line_log="std::log(float)" if _one_of(names["LINES"], "logf", "log", "MapLine::PredictScale") else "::log(double)",
                     atan2="atan2f" if _one_of(names["LINES"], "atan2f", "atan2", "GetLine2dRepresentation") else "atan2")
    pl.ref_kf_create.restype = _vp
    pl.ref_kf_create.argtypes = [_i] + [_vp] * 6 + [_f, _f, _vp, _f, _vp, _vp, _f, _vp, _vp, _i, _vp, _vp, _f]
    pl.ref_kf_destroy.argtypes = [_vp]
    pl.ref_kf_destroy.restype = None
    pl.ref_fuse.restype = _i
    pl.ref_fuse.argtypes = [_vp, _i] + [_vp] * 6 + [_f] + [_vp] * 5
    pl.ref_fuse_plain.restype = _i
    pl.ref_fuse_plain.argtypes = [_vp, _i] + [_vp] * 6 + [_f]
    ll.ref_line_kf_create.restype = _vp
    ll.ref_line_kf_create.argtypes = [_i] + [_vp] * 6 + [_f, _vp, _f, _vp, _vp, _f, _i, _vp, _vp, _f]
    ll.ref_line_kf_destroy.argtypes = [_vp]
    ll.ref_line_kf_destroy.restype = None
    ll.ref_line_pose.argtypes = [_vp, _vp, _vp]
    ll.ref_line_pose.restype = None
    ll.ref_line_fuse.restype = _i
    ll.ref_line_fuse.argtypes = [_vp, _i] + [_vp] * 6 + [_f, _vp, _vp, _vp]
    ll.ref_line_fuse_plain.restype = _i
    ll.ref_line_fuse_plain.argtypes = [_vp, _i] + [_vp] * 6 + [_f]
    ll.ref_chi_square.restype = _f
    defines = dict(USE_ENDPOINTS_AVERAGING=ll.ref_use_endpoints_averaging(),
                   USE_DISTSEGMENT2SEGMENT_FOR_MATCHING=ll.ref_use_distsegment2segment(), TH_LOW_lines=ll.ref_th_low(),
                   kChiSquareLinePointProj=float(ll.ref_chi_square()))
    assert defines["USE_ENDPOINTS_AVERAGING"] == 0, "MapLine::Replace averages end points: the replay rule of INTEGRATION 2l no longer holds"
    assert defines["USE_DISTSEGMENT2SEGMENT_FOR_MATCHING"] == 0 and defines["TH_LOW_lines"] == LR.TH_LOW
    assert np.float32(defines["kChiSquareLinePointProj"]) == LR.CHI2
    return pl, ll, overloads, defines


def point_kf_create(lib, kf):
    keep = [np.ascontiguousarray(kf[k], t) for k, t in (("x", np.float32), ("y", np.float32), ("octave", np.int32), ("u_right", np.float32),
                                                       ("desc", np.uint8), ("bounds4", np.float32), ("K4", np.float32), ("Rcw", np.float32),
                                                       ("s_t", np.float32), ("q_cw", np.float32), ("Ow_points", np.float32),
                                                       ("scale_factors", np.float32), ("inv_level_sigma2", np.float32))]
    x, y, octv, ur, desc, b4, K4, Rcw, s_t, q, Ow, sf, sig = keep
    assert (b4 == np.round(b4)).all() and b4[0] == kf["min_x"] and b4[2] == kf["min_y"], "the key frame holds its bounds as int"
    h = lib.ref_kf_create(len(x), _p(x), _p(y), _p(octv), _p(ur), _p(desc), _p(b4), float(kf["grid_w_inv"]), float(kf["grid_h_inv"]), _p(K4),
                          float(kf["mbf"]), _p(Rcw), _p(s_t), float(kf["scale"]), _p(q), _p(Ow), len(sf), _p(sf), _p(sig),
                          float(kf["log_scale_factor"]))
    return h, keep


def ref_point_fuse(lib, inp):
    """The reference's Fuse, one call per key frame -> the restatement's fields as far as the accessors record them."""
    GOT_WORLD_POS, PROJECTED, GOT_MAX_DISTANCE, GOT_NORMAL, GOT_DESCRIPTOR, GOT_MAP_POINT, ADD_OBSERVATION, ADD_MAP_POINT, REPLACE = (1 << b for b in range(9))
    pts, K = inp["points"], len(inp["kfs"])
    M = len(pts["min_dist"])
    o = dict(reached=np.zeros((K, M), np.uint8), raw_best_idx=np.full((K, M), -1, np.int32), raw_best_dist=np.full((K, M), 256, np.int32),
             n_dist=np.zeros((K, M), np.int32), u=np.zeros((K, M), np.float32), v=np.zeros((K, M), np.float32), n_fused=np.zeros(K, np.int32))
    for k, kf in enumerate(inp["kfs"]):
        h, keep = point_kf_create(lib, kf)
        rec, uv, band = np.zeros((M, 4), np.int32), np.zeros((M, 2), np.float32), np.zeros(M, np.int32)
        tcw, replaced = np.zeros(3, np.float32), np.zeros(max(M, 1), np.uint8)
        sk = None if inp["skip"] is None else np.ascontiguousarray(inp["skip"][k])
        o["n_fused"][k] = lib.ref_fuse(h, M, _p(pts["pos"]), _p(pts["normal"]), _p(pts["min_dist"]), _p(pts["max_dist"]), _p(pts["desc"]), _p(sk),
                                       float(inp["th"]), _p(rec), _p(uv), _p(band), _p(tcw), _p(replaced))
        lib.ref_kf_destroy(h)
        assert same(tcw, np.asarray(kf["tcw"], np.float32)), f"key frame {k}: the compiled Scw.translation() / Scw.scale() is not the scenario's tcw"
        assert not replaced.any(), "GetMapPoint returns null: nothing to replace"
        for i in range(M):
            fl, nd, md, bi = (int(c) for c in rec[i])
            if not fl & GOT_WORLD_POS:
                r = PR.SKIPPED
            elif not fl & PROJECTED:
                r = PR.BEHIND
            elif not fl & GOT_MAX_DISTANCE:
                r = PR.OUTSIDE
            elif not fl & GOT_NORMAL:
                assert band[i] in (1, 2), "stopped at the band, and neither comparison of :1489 holds"
                r = PR.TOO_NEAR if band[i] == 1 else PR.TOO_FAR
            elif not fl & GOT_DESCRIPTOR:
                r = None           # the viewing angle (:1495) or the empty window (:1506): the restatement, compared below, tells
            elif nd == 0:
                r = PR.NO_CANDIDATE
            elif fl & GOT_MAP_POINT:
                assert fl & ADD_OBSERVATION and fl & ADD_MAP_POINT and not fl & REPLACE and md <= PR.TH_LOW
                r = PR.CANDIDATE
            else:
                assert md > PR.TH_LOW
                r = PR.ABOVE_TH_LOW
            o["reached"][k, i] = 255 if r is None else r
            o["n_dist"][k, i] = nd
            if fl & PROJECTED:
                o["u"][k, i], o["v"][k, i] = uv[i]
            if nd:
                o["raw_best_dist"][k, i] = md
            if fl & GOT_MAP_POINT:
                o["raw_best_idx"][k, i] = bi
        assert o["n_fused"][k] == int((o["reached"][k] == PR.CANDIDATE).sum())
    return o


def compare_points(ref, rest, name):
    open_ = ref["reached"] == 255
    assert np.isin(rest["reached"][open_], (PR.VIEW_ANGLE, PR.EMPTY_WINDOW)).all(), name
    assert same(np.where(open_, rest["reached"], ref["reached"]), rest["reached"]), f"{name}: reached differs at {np.argwhere(ref['reached'] != rest['reached'])[:8]}"
    for k in ("n_dist", "raw_best_dist", "u", "v"):
        assert same(ref[k], rest[k]), f"{name}: {k} differs at {np.argwhere(ref[k] != rest[k])[:8]}"
    assert same(ref["raw_best_idx"], rest["best_idx"]), f"{name}: bestIdx differs"
    out = dict(ref)
    out["reached"] = rest["reached"].copy()
    return out


def line_kf_create(lib, kf):
    kl = kf["kl"]
    segs = np.ascontiguousarray(np.stack([kl["startPointX"], kl["startPointY"], kl["endPointX"], kl["endPointY"]], 1), np.float32).reshape(-1, 4)
    octv = np.ascontiguousarray(kl["octave"], np.int32)
    f = lambda k: None if kf[k] is None else np.ascontiguousarray(kf[k], np.float32)
    keep = [segs, octv, f("u_right_start"), f("u_right_end"), np.ascontiguousarray(kf["desc"], np.uint8), f("bounds4"), f("K4"), f("Rcw"), f("s_t"),
            f("scale_factors"), f("inv_level_sigma2")]
    assert (keep[5] == np.round(keep[5])).all(), "the key frame holds its bounds as int"
    h = lib.ref_line_kf_create(len(kl), _p(segs), _p(octv), _p(keep[2]), _p(keep[3]), _p(keep[4]), _p(keep[5]), float(kf["max_diag"]), _p(keep[6]),
                               float(kf["mbf"]), _p(keep[7]), _p(keep[8]), float(kf["scale"]), len(keep[9]), _p(keep[9]), _p(keep[10]),
                               float(kf["log_scale_factor"]))
    return h, keep


def ref_line_fuse(lib, inp):
    GOT_END_POINTS, GOT_MAX_DISTANCE, GOT_NORMAL, PREDICTED, GOT_DESCRIPTOR, GOT_MAP_LINE, ADD_OBSERVATION, ADD_MAP_LINE, REPLACE = (1 << b for b in range(9))
    ln, K = inp["lines"], len(inp["kfs"])
    M = len(ln["max_dist"])
    o = dict(reached=np.zeros((K, M), np.uint8), raw_best_idx=np.full((K, M), -1, np.int32), raw_best_dist=np.full((K, M), 256, np.int32),
             n_dist=np.zeros((K, M), np.int32), level=np.full((K, M), -1, np.int32), proj=np.zeros((K, M, 6), np.float32),
             n_proj=np.zeros((K, M), np.int32), n_fused=np.zeros(K, np.int32))
    for k, kf in enumerate(inp["kfs"]):
        h, keep = line_kf_create(lib, kf)
        tcw, ow = np.zeros(3, np.float32), np.zeros(3, np.float32)
        lib.ref_line_pose(h, _p(tcw), _p(ow))
        assert same(tcw, np.asarray(kf["tcw"], np.float32)), f"key frame {k}: the compiled Scw.translation() / scale is not the scenario's tcw"
        assert same(ow, np.asarray(kf["Ow_lines"], np.float32)), f"key frame {k}: the compiled -Rcw.transpose() * tcw is not the scenario's Ow_lines"
        rec, proj, stop = np.zeros((M, 6), np.int32), np.zeros((M, 6), np.float32), np.zeros(M, np.int32)
        sk = None if inp["skip"] is None else np.ascontiguousarray(inp["skip"][k])
        o["n_fused"][k] = lib.ref_line_fuse(h, M, _p(ln["start"]), _p(ln["end"]), _p(ln["normal"]), _p(ln["max_dist"]), _p(ln["desc"]), _p(sk),
                                            float(inp["th"]), _p(rec), _p(proj), _p(stop))
        lib.ref_line_kf_destroy(h)
        for i in range(M):
            fl, npj, nd, md, bi, lv = (int(c) for c in rec[i])
            if not fl & GOT_END_POINTS:
                r = LR.SKIPPED
            elif npj == 0:
                r = LR.MIDDLE_BEHIND
            elif not fl & GOT_MAX_DISTANCE:
                r = LR.MIDDLE_OUTSIDE
            elif not fl & GOT_NORMAL:
                r = {1: LR.TOO_NEAR, 2: LR.TOO_FAR, 3: LR.END_BEHIND, 4: LR.END_OUTSIDE}[int(stop[i])]
            elif not fl & PREDICTED:
                r = LR.VIEW_ANGLE
            elif not fl & GOT_DESCRIPTOR:
                r = LR.EMPTY_WINDOW
            elif nd == 0:
                r = LR.NO_CANDIDATE
            elif fl & GOT_MAP_LINE:
                assert fl & ADD_OBSERVATION and fl & ADD_MAP_LINE and not fl & REPLACE and md <= LR.TH_LOW
                r = LR.CANDIDATE
            else:
                assert md > LR.TH_LOW
                r = LR.ABOVE_TH_LOW
            o["reached"][k, i], o["n_dist"][k, i], o["level"][k, i], o["n_proj"][k, i] = r, nd, lv, min(npj, 3)
            o["proj"][k, i] = proj[i]
            if nd:
                o["raw_best_dist"][k, i] = md
            if fl & GOT_MAP_LINE:
                o["raw_best_idx"][k, i] = bi
        assert o["n_fused"][k] == int((o["reached"][k] == LR.CANDIDATE).sum())
    return o


def compare_lines(ref, rest, name):
    for k in ("reached", "n_dist", "raw_best_dist", "level", "n_proj", "proj"):
        assert same(ref[k], rest[k]), f"{name}: {k} differs at {np.argwhere(ref[k] != rest[k])[:8].tolist()}"
    assert same(ref["raw_best_idx"], rest["best_idx"]), f"{name}: bestIdx differs"
    return ref


def time_reference(pl, ll):
    """One core, the measurement's loop shape: every key frame's two Fuse calls, as SearchAndFuse makes them."""
    out = {}
    for kind, inp, lib, create, destroy, plain, items, keys in (
            ("points", S.nominal_point_inputs(), pl, point_kf_create, pl.ref_kf_destroy, pl.ref_fuse_plain, "points",
             ("pos", "normal", "min_dist", "max_dist", "desc")),
            ("lines", S.nominal_line_inputs(), ll, line_kf_create, ll.ref_line_kf_destroy, ll.ref_line_fuse_plain, "lines",
             ("start", "end", "normal", "max_dist", "desc"))):
        it = inp[items]
        M = len(it["max_dist"])
        args = [_p(it[k]) for k in keys]
        us = []
        for rep in range(7):
            t0 = time.perf_counter()
            for k, kf in enumerate(inp["kfs"]):
                h, keep = create(lib, kf)
                plain(h, M, *args, _p(np.ascontiguousarray(inp["skip"][k])), float(inp["th"]))
                destroy(h)
            if rep >= 2:
                us.append((time.perf_counter() - t0) * 1e6)
        K, N = len(inp["kfs"]), len(inp["kfs"][0]["x" if kind == "points" else "kl"])
        out[kind] = dict(shape=[K, M, N], us_median=round(float(np.median(us)), 1), us_min=round(float(np.min(us)), 1),
                         us_max=round(float(np.max(us)), 1))
    out["what"] = ("the reference's two Sim3 Fuse overloads as compiled by scripts/make_loop_fuse_golden.py (-O2, no contraction), one call per "
                   "key frame at tests/loop_fuse_scenario.nominal_point_inputs() / nominal_line_inputs(), one core, wall clock incl. filling the "
                   "objects and the grids; median, min and max of 5 after 2")
    out["machine"] = f"{_cpu_model()}, {os.cpu_count()} logical CPUs (the host that ran this script, not the MI355X host of the GPU figures)"
    out["source"] = "scripts/make_loop_fuse_golden.py --time"
    return out


def main():
    with tempfile.TemporaryDirectory() as tmp:
        pl, ll, overloads, defines = build_wrappers(tmp)
        pd, ld, ad = overloads["point_log"] != "std::log(float)", overloads["line_log"] != "std::log(float)", overloads["atan2"] != "atan2f"
        # ---- points
        inp, crowd = S.point_inputs(), S.crowd_point_inputs()
        pc, pcc, pca = {}, {}, {}
        ref_p = compare_points(ref_point_fuse(pl, inp), R.point_search(inp["kfs"], inp["points"], inp["skip"], inp["th"], pc, pd), "points")
        ref_pc = compare_points(ref_point_fuse(pl, crowd), R.point_search(crowd["kfs"], crowd["points"], None, crowd["th"], pcc, pd), "point crowd")
        for rnd in (S.random_point_inputs(3, 120, 150, seed=3), S.ambiguous_point_inputs()):
            compare_points(ref_point_fuse(pl, rnd), R.point_search(rnd["kfs"], rnd["points"], rnd["skip"], rnd["th"], pca, pd), "random points")
        assert pca["ambiguous"] >= 1
        # ---- lines
        linp, lcrowd = S.line_inputs(), S.crowd_line_inputs()
        lc, lcc, lca = {}, {}, {}
        ref_l = compare_lines(ref_line_fuse(ll, linp), R.line_search(linp["kfs"], linp["lines"], linp["skip"], linp["th"], lc, ld, ad), "lines")
        ref_lc = compare_lines(ref_line_fuse(ll, lcrowd), R.line_search(lcrowd["kfs"], lcrowd["lines"], None, lcrowd["th"], lcc, ld, ad), "line crowd")
        for rnd in (S.random_line_inputs(3, 120, 150, seed=3), S.ambiguous_line_inputs()):
            compare_lines(ref_line_fuse(ll, rnd), R.line_search(rnd["kfs"], rnd["lines"], rnd["skip"], rnd["th"], lca, ld, ad), "random lines")
        assert lca["ambiguous_level"] >= 1 and lca["ambiguous_theta"] >= 1
        timing = time_reference(pl, ll) if "--time" in sys.argv else None
    # ---- every stage and every placed case is reached in the compiled run: conditions on the scenario
    for k in PR.REACHED + tuple(f for f in R.POINT_SUB_FACTS if f != "dist3d_zero"):
        assert pc[k] >= 1, f"the reference's point run does not take {k}: {pc}"
    w = inp["where"]
    rk = lambda name, k=0: [int(ref_p["reached"][k, i]) for i in w[name]]
    expect = dict(candidate_mono=PR.CANDIDATE, candidate_stereo=PR.CANDIDATE, candidate_level_minus_1=PR.CANDIDATE, below_level=PR.NO_CANDIDATE,
                  above_level=PR.NO_CANDIDATE, mono_gate=PR.CANDIDATE, stereo_gate=PR.CANDIDATE, u_right_zero=PR.CANDIDATE,
                  chi2_far=PR.CANDIDATE, chi2_stereo_far=PR.CANDIDATE, above_th_low=PR.ABOVE_TH_LOW, tie=PR.CANDIDATE, clip_left=PR.CANDIDATE,
                  clip_right=PR.CANDIDATE, clip_top=PR.CANDIDATE, clip_bottom=PR.CANDIDATE, empty_window=PR.EMPTY_WINDOW, behind=PR.BEHIND,
                  outside=PR.OUTSIDE, too_near=PR.TOO_NEAR, too_far=PR.TOO_FAR, view_angle=PR.VIEW_ANGLE, skip_null=PR.SKIPPED, skip_bad=PR.SKIPPED)
    for name, code in expect.items():
        assert all(r == code for r in rk(name)), f"{name}: the reference's run reached {rk(name)}, not {code}"
    assert rk("skip_in_kf", 0)[0] == PR.SKIPPED and rk("skip_in_kf", 2)[1] == PR.SKIPPED and rk("skip_in_kf", 1)[0] != PR.SKIPPED
    ja, jb = w["tie_indices"]
    assert ja > jb and int(ref_p["raw_best_idx"][0, w["tie"][0]]) == ja, "the tie's winner is not the higher index"
    for name in ("z_zero_nan", "z_zero_inf"):
        i = w[name][0]
        assert ref_p["reached"][2, i] == PR.OUTSIDE and not np.isfinite(ref_p["u"][2, i]), name
    assert np.isnan(ref_p["u"][2, w["z_zero_nan"][0]]) and np.isinf(ref_p["u"][2, w["z_zero_inf"][0]])
    assert pcc["tie_winner_not_lowest_index"] >= 1 and pcc["candidate"] == 8
    # the compiled Sim3 cut takes the two far candidates AND the SE3 restatement, on the same poses, rejects them
    se3 = PR.fuse_search([R.point_kf(kf) for kf in inp["kfs"]], inp["points"], inp["skip"], inp["th"], None, pd)
    for name, member in zip(("chi2_far", "chi2_stereo_far"), w["chi2_members"]):
        i = w[name][0]
        assert int(ref_p["raw_best_idx"][0, i]) == member and int(se3["reached"][0, i]) == PR.NO_CANDIDATE, name
    for k in LR.REACHED + R.LINE_SUB_FACTS:
        if k in ("degenerate", "dist_zero", "end_points_coincide", "beyond_member_64"):
            assert lc[k] == 0, k            # undefined in the reference: not in its run; the crowd's own
            continue
        assert lc[k] >= 1, f"the reference's line run does not take {k}: {lc}"
    assert lcc["beyond_member_64"] >= 1 and lcc["candidate"] == 8
    lw = linp["where"]
    lrk = lambda name, k=0: [int(ref_l["reached"][k, i]) for i in lw[name]]
    lexpect = dict(candidate_mono=LR.CANDIDATE, above_level=LR.NO_CANDIDATE, below_level=LR.NO_CANDIDATE, start_gate=LR.NO_CANDIDATE,
                   end_gate=LR.NO_CANDIDATE, right_gate=LR.CANDIDATE, u_right_start_zero=LR.CANDIDATE, u_right_end_negative=LR.CANDIDATE,
                   sigma_level=LR.CANDIDATE, right_far=LR.CANDIDATE, dist_60=LR.CANDIDATE, dist_61=LR.ABOVE_TH_LOW, empty_window=LR.EMPTY_WINDOW,
                   clip_column_0=LR.CANDIDATE, clip_column_159=LR.CANDIDATE, split_minus=LR.CANDIDATE, split_plus_tie=LR.CANDIDATE,
                   middle_behind=LR.MIDDLE_BEHIND, middle_outside=LR.MIDDLE_OUTSIDE, too_near=LR.TOO_NEAR, too_far=LR.TOO_FAR,
                   end_behind=LR.END_BEHIND, end_outside=LR.END_OUTSIDE, view_angle=LR.VIEW_ANGLE, skip_null=LR.SKIPPED, skip_bad=LR.SKIPPED)
    for name, code in lexpect.items():
        assert all(r == code for r in lrk(name)), f"{name}: the reference's run reached {lrk(name)}, not {code}"
    assert lrk("window_misses_grid", 2) == [LR.EMPTY_WINDOW]
    assert lrk("skip_in_kf", 1)[0] == LR.SKIPPED and lrk("skip_in_kf", 2)[1] == LR.SKIPPED and lrk("skip_in_kf", 0)[0] != LR.SKIPPED
    assert int(ref_l["raw_best_dist"][0, lw["dist_60"][0]]) == 60 and int(ref_l["raw_best_dist"][0, lw["dist_61"][0]]) == 61
    ja, jb = lw["tie_indices"]
    assert ja > jb and int(ref_l["raw_best_idx"][0, lw["split_plus_tie"][0]]) == ja, "the tie's winner is not the higher index"
    assert int(ref_l["raw_best_idx"][0, lw["split_minus"][0]]) == lw["split_minus_members"][0]
    lse3 = LR.fuse_search([R.line_kf(kf) for kf in linp["kfs"]], linp["lines"], linp["skip"], linp["th"], None, ld, ad)
    for name, member in zip(("sigma_level", "right_far"), lw["sim3_members"]):
        i = lw[name][0]
        assert int(ref_l["raw_best_idx"][0, i]) == member and int(lse3["reached"][0, i]) == LR.NO_CANDIDATE, name
    assert lc["taken_where_kl_level_sigma_drops"] >= 1 and lc["taken_where_right_gate_drops"] >= 1
    facts = dict(point_counts=pc, point_crowd_counts=pcc, line_counts=lc, line_crowd_counts=lcc,
                 ambiguous_counts=dict(points=pca["ambiguous"], line_level=lca["ambiguous_level"], line_theta=lca["ambiguous_theta"]),
                 overloads=overloads, double_overloads=dict(point_log=int(pd), line_log=int(ld), atan2=int(ad)), defines=defines,
                 n_fused=dict(points=[int(n) for n in ref_p["n_fused"]], lines=[int(n) for n in ref_l["n_fused"]]),
                 point_where={k: [int(i) for i in v] for k, v in w.items()}, line_where={k: [int(i) for i in v] for k, v in lw.items()})
    gdir = os.path.join(ROOT, "tests", "golden")
    digests = dict(point_inputs=S.digest(inp), point_crowd_inputs=S.digest(crowd), line_inputs=S.digest(linp), line_crowd_inputs=S.digest(lcrowd))
    arrays = {}
    for pre, src in (("point_", ref_p), ("point_crowd_", ref_pc), ("line_", ref_l), ("line_crowd_", ref_lc)):
        arrays.update({pre + k: v for k, v in src.items()})
    np.savez_compressed(os.path.join(gdir, "loop_fuse_reference.npz"), **arrays, **{k + "_digest": np.array(v) for k, v in digests.items()})
    with open(os.path.join(gdir, "loop_fuse_reference_facts.json"), "w") as fh:
        json.dump(dict(what="branch counts of the reference's two Sim3 Fuse overloads on tests/loop_fuse_scenario.py (the restatement's "
                            "counters, taken only after the restatement reproduced the compiled cuts bit for bit), the `log` and `atan2` "
                            "overloads they were compiled with, the #defines and the placed cases (see scripts/make_loop_fuse_golden.py); "
                            "Eigen's decomposition of Scw is outside the pin", digests=digests, facts=facts), fh, indent=1)
    if timing:
        tpath = os.path.join(ROOT, "profiles", "loop_fuse_timing.json")
        doc = {}
        if os.path.exists(tpath):
            with open(tpath) as fh:
                doc = json.load(fh)
        doc["cpu_reference"] = timing
        with open(tpath, "w") as fh:
            json.dump(doc, fh, indent=1)
    print(json.dumps(facts)[:2000], timing)


if __name__ == "__main__":
    main()
