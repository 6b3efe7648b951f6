#!/usr/bin/env python3
"""Golden outputs of the REFERENCE'S OWN LineMatcher::Fuse(pKF, vpMapLines, th, bRight = false) on tests/line_fuse_scenario.py.  The
definitions — LineMatcher::Fuse (src/LineMatcher.cc:2043-2315), both KeyFrame::GetLineFeaturesInArea overloads it reaches
(src/KeyFrame.cc:1291-1402), LineProjection::ProjectLineWithCheck (include/LineProjection.h:144-264),
Geom2DUtils::GetLine2dRepresentation(NoTheta) (include/Geom2DUtils.h:135-159), MapLine::PredictScale(const float&, KeyFramePtr&)
(src/MapLine.cc:721-736), the two distance-invariance getters (:707-719), GeometricCamera::projectLinear(const Eigen::Vector3f&), the
constants and the #defines of src/LineMatcher.cc:38-40 and src/MapLine.cc:33 — are cut verbatim out of the reference tree into a
temporary directory at build time and compiled around scripts/ref_wrap/line_fuse_ref_wrap.cpp (declarations, recording accessors,
calls and labelled restatements) against oracle/ref/eigen_full with -O2 -ffp-contract=off -fno-fast-math.  What each pair did comes
from the accessors the compiled text called.  Writes
  tests/golden/line_fuse_reference.npz          reached, bestIdx, bestDist, distances taken, level, projections per pair, which key
                                                lines PosLineInGrid placed + the inputs digests
  tests/golden/line_fuse_reference_facts.json   per-branch counts, the `log` and `atan2` overloads compiled, the #defines, the
                                                placed cases
and, with --time, the compiled cut's time on one core at 30 key frames x 300 lines x 300 key lines
(profiles/line_fuse_timing.json, key "cpu_reference").  Dev-time tool: needs the reference tree.  Changes nothing under oracle/.

The replay rule of INTEGRATION.md 2j rests on USE_ENDPOINTS_AVERAGING == 0 (src/MapLine.cc:33): with it, MapLine::Replace moves no
end point, normal or mfMaxDistance inside the loop.  This script asserts the #define it cut is 0 and records it."""
import ctypes
import json
import os
import platform
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from scripts.make_frame_rgbd_golden import reference_root      # noqa: E402
from tests import line_fuse_restatement as R                   # noqa: E402
from tests import line_fuse_scenario as S                      # noqa: E402

_vp, _i, _f = ctypes.c_void_p, ctypes.c_int, ctypes.c_float
CUTS = {"line_fuse_cut_macros.inc": (
            ("include/Frame.h", r"/^#define LINE_THETA_SPAN /,/^#define LINE_D_GRID_COLS /"),
            ("src/LineMatcher.cc", r"/^#define USE_DISTSEGMENT2SEGMENT_FOR_MATCHING /,/^#define USE_STEREO_PROJECTION_CHECK /"),
            ("src/MapLine.cc", r"/^#define USE_ENDPOINTS_AVERAGING /")),
        "line_fuse_cut_geom.inc": (
            ("include/Geom2DUtils.h", r"/^    static void GetLine2dRepresentationNoTheta\(/,/^    }/"),
            ("include/Geom2DUtils.h", r"/^    static void GetLine2dRepresentation\(/,/^    }/")),
        "line_fuse_cut_accessors.inc": (
            ("include/CameraModels/GeometricCamera.h", r"/^    inline Eigen::Vector2f GeometricCamera::projectLinear\(const Eigen::Vector3f/,/^    }/"),
            ("src/MapLine.cc", r"/^float MapLine::GetMinDistanceInvariance/,/^}/"),
            ("src/MapLine.cc", r"/^float MapLine::GetMaxDistanceInvariance/,/^}/"),
            ("src/MapLine.cc", r"/^int MapLine::PredictScale\(const float &currentDist, KeyFramePtr& pKF\)/,/^}/")),
        "line_fuse_cut_lineproj.inc": (("include/LineProjection.h", r"/^inline bool LineProjection::ProjectLineWithCheck/,/^}/"),),
        "line_fuse_cut_defs.inc": (
            ("src/LineMatcher.cc", r"/^const float kChiSquareLinePointProj = /"),
            ("src/LineMatcher.cc", r"/^const int LineMatcher::TH_LOW = /"),
            ("src/Frame.cc", r"/^const float Frame::kDeltaTheta = /"),
            ("src/Frame.cc", r"/^const float Frame::kDeltaD = /"),
            ("src/KeyFrame.cc", r"/^vector<size_t> KeyFrame::GetLineFeaturesInArea\(const Line2DRepresentation& lineRepresentation/,/^}/"),
            ("src/KeyFrame.cc", r"/^void KeyFrame::GetLineFeaturesInArea\(const float thetaMin/,/^}/"),
            ("src/LineMatcher.cc", r"/^int LineMatcher::Fuse\(KeyFramePtr& pKF, const vector<MapLinePtr> &vpMapLines, const float th, const bool bRight\)/,/^}/"))}
GOT_END_POINTS, GOT_MAX_DISTANCE, GOT_NORMAL, PREDICTED, GOT_DESCRIPTOR, GOT_MAP_LINE, ADD_OBSERVATION, ADD_MAP_LINE, REPLACE = (1 << b for b in range(9))
TIMING_SHAPE = (30, 300, 300)


def _p(a):
    return None if a is None else np.ascontiguousarray(a).ctypes.data_as(_vp)


def _one_of(names, f32_name, f64_name, what):
    assert (f32_name in names) != (f64_name in names), f"the compiled {what} calls neither or both of {f32_name} / {f64_name}"
    return f32_name in names


def build_wrapper(tmp):
    ref, oref = reference_root(), os.path.join(ROOT, "oracle", "ref")
    for name, cuts in CUTS.items():
        with open(os.path.join(tmp, name), "w") as out:
            for path, pattern in cuts:
                text = subprocess.run(["awk", pattern, os.path.join(ref, path)], check=True, capture_output=True, text=True).stdout
                assert text.strip(), f"nothing cut from {path} by {pattern}"
                out.write(text + "\n")
    so = os.path.join(tmp, "libline_fuse_ref.so")
    subprocess.run(["g++", "-O2", "-std=c++14", "-fPIC", "-ffp-contract=off", "-fno-fast-math", "-w", "-I" + os.path.join(oref, "eigen_full"),
                    "-I" + tmp, "-shared", os.path.join(ROOT, "scripts", "ref_wrap", "line_fuse_ref_wrap.cpp"), "-o", so], check=True)
    undefined = subprocess.run(["nm", "-D", "--undefined-only", so], check=True, capture_output=True, text=True).stdout.split()
    names = {u.split("@")[0] for u in undefined}
    overloads = dict(log="std::log(float)" if _one_of(names, "logf", "log", "PredictScale") else "::log(double)",
                     atan2="atan2f" if _one_of(names, "atan2f", "atan2", "GetLine2dRepresentation") else "atan2")
    lib = ctypes.CDLL(so)
    lib.ref_line_kf_create.restype = _vp
    lib.ref_line_kf_create.argtypes = [_i] + [_vp] * 6 + [_f, _vp, _f, _vp, _vp, _vp, _i, _vp, _vp, _f, _vp]
    lib.ref_line_kf_destroy.argtypes = [_vp]
    lib.ref_line_kf_destroy.restype = None
    lib.ref_line_fuse.restype = _i
    lib.ref_line_fuse.argtypes = [_vp, _i] + [_vp] * 6 + [_f, _vp, _vp, _vp]
    lib.ref_line_fuse_plain.restype = _i
    lib.ref_line_fuse_plain.argtypes = [_vp, _i] + [_vp] * 6 + [_f]
    lib.ref_line_predict_scale.restype = _i
    lib.ref_line_predict_scale.argtypes = [_f, _f, _f, _i]
    lib.ref_line_theta.restype = _f
    lib.ref_line_theta.argtypes = [_f] * 4
    lib.ref_chi_square.restype = _f
    defines = dict(USE_ENDPOINTS_AVERAGING=lib.ref_use_endpoints_averaging(), USE_DISTSEGMENT2SEGMENT_FOR_MATCHING=lib.ref_use_distsegment2segment(),
                   USE_STEREO_PROJECTION_CHECK=lib.ref_use_stereo_projection_check(), TH_LOW=lib.ref_th_low(),
                   kChiSquareLinePointProj=float(lib.ref_chi_square()))
    assert defines["USE_ENDPOINTS_AVERAGING"] == 0, "MapLine::Replace averages end points: the replay rule of INTEGRATION 2j no longer holds"
    assert defines["USE_DISTSEGMENT2SEGMENT_FOR_MATCHING"] == 0 and defines["USE_STEREO_PROJECTION_CHECK"] == 1 and defines["TH_LOW"] == R.TH_LOW
    assert np.float32(defines["kChiSquareLinePointProj"]) == R.CHI2
    return lib, overloads, defines


def kf_create(lib, kf):
    kl = kf["kl"]
    segs = np.ascontiguousarray(np.stack([kl["startPointX"], kl["startPointY"], kl["endPointX"], kl["endPointY"]], 1), np.float32).reshape(-1, 4)
    octv = np.ascontiguousarray(kl["octave"], np.int32)
    f = lambda k: None if kf[k] is None else np.ascontiguousarray(kf[k], np.float32)
    keep = [segs, octv, f("u_right_start"), f("u_right_end"), np.ascontiguousarray(kf["desc"], np.uint8), f("bounds4"), f("K4"), f("Rcw"), f("tcw"),
            f("Ow"), f("scale_factors"), f("inv_level_sigma2"), np.zeros(max(len(kl), 1), np.uint8)]
    b4 = keep[5]
    assert (b4 == np.round(b4)).all(), "the key frame holds its bounds as int"
    h = lib.ref_line_kf_create(len(kl), _p(segs), _p(octv), _p(keep[2]), _p(keep[3]), _p(keep[4]), _p(b4), float(kf["max_diag"]), _p(keep[6]),
                               float(kf["mbf"]), _p(keep[7]), _p(keep[8]), _p(keep[9]), len(keep[10]), _p(keep[10]), _p(keep[11]),
                               float(kf["log_scale_factor"]), _p(keep[12]))
    return h, keep


def ref_fuse(lib, inp):
    """The reference's Fuse, one call per key frame -> the restatement's fields as the accessors record them."""
    ln, K = inp["lines"], len(inp["kfs"])
    M = len(ln["max_dist"])
    o = dict(reached=np.zeros((K, M), np.uint8), raw_best_idx=np.full((K, M), -1, np.int32), raw_best_dist=np.full((K, M), 256, np.int32),
             n_dist=np.zeros((K, M), np.int32), level=np.full((K, M), -1, np.int32), proj=np.zeros((K, M, 6), np.float32),
             n_proj=np.zeros((K, M), np.int32), n_fused=np.zeros(K, np.int32))
    in_grid = []
    for k, kf in enumerate(inp["kfs"]):
        h, keep = kf_create(lib, kf)
        in_grid.append(keep[12][:len(kf["kl"])].copy())
        rec, proj, stop = np.zeros((M, 6), np.int32), np.zeros((M, 6), np.float32), np.zeros(M, np.int32)
        sk = None if inp["skip"] is None else np.ascontiguousarray(inp["skip"][k])
        o["n_fused"][k] = lib.ref_line_fuse(h, M, _p(ln["start"]), _p(ln["end"]), _p(ln["normal"]), _p(ln["max_dist"]), _p(ln["desc"]), _p(sk),
                                            float(inp["th"]), _p(rec), _p(proj), _p(stop))
        lib.ref_line_kf_destroy(h)
        for i in range(M):
            fl, npj, nd, md, bi, lv = (int(c) for c in rec[i])
            if not fl & GOT_END_POINTS:
                r = R.SKIPPED
            elif npj == 0:
                r = R.MIDDLE_BEHIND
            elif not fl & GOT_MAX_DISTANCE:
                r = R.MIDDLE_OUTSIDE
            elif not fl & GOT_NORMAL:
                r = {1: R.TOO_NEAR, 2: R.TOO_FAR, 3: R.END_BEHIND, 4: R.END_OUTSIDE}[int(stop[i])]
            elif not fl & PREDICTED:
                r = R.VIEW_ANGLE
            elif not fl & GOT_DESCRIPTOR:
                r = R.EMPTY_WINDOW
            elif nd == 0:
                r = R.NO_CANDIDATE
            elif fl & GOT_MAP_LINE:
                assert fl & ADD_OBSERVATION and fl & ADD_MAP_LINE and not fl & REPLACE and md <= R.TH_LOW
                r = R.CANDIDATE
            else:
                assert md > R.TH_LOW
                r = R.ABOVE_TH_LOW
            o["reached"][k, i], o["n_dist"][k, i], o["level"][k, i], o["n_proj"][k, i] = r, nd, lv, min(npj, 3)
            o["proj"][k, i] = proj[i]
            if nd:
                o["raw_best_dist"][k, i] = md
            if fl & GOT_MAP_LINE:
                o["raw_best_idx"][k, i] = bi
        assert o["n_fused"][k] == int((o["reached"][k] == R.CANDIDATE).sum())
    return o, in_grid


def same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def compare(ref, in_grid, rest, kfs, name):
    """The restatement against the compiled cut, bit for bit.  bestIdx is observable where bestDist <= TH_LOW only."""
    for k in ("reached", "n_dist", "raw_best_dist", "level", "n_proj", "proj"):
        assert same(ref[k], rest[k]), f"{name}: {k} differs at {np.argwhere(ref[k] != rest[k])[:8].tolist()}"
    assert same(ref["raw_best_idx"], rest["best_idx"]), f"{name}: bestIdx differs"
    for kf, placed in zip(kfs, in_grid):
        mine = np.zeros(len(kf["kl"]), np.uint8)
        mine[R.grid_of(kf)[1]] = 1
        assert same(mine, placed), f"{name}: PosLineInGrid differs at {np.flatnonzero(mine != placed)[:8].tolist()}"
    return ref


def _cpu_model():
    try:
        with open("/proc/cpuinfo") as fh:
            for line in fh:
                if line.startswith("model name"):
                    return line.split(":", 1)[1].strip()
    except OSError:
        pass
    return platform.processor() or platform.machine()


def time_reference(lib):
    K, M, N = TIMING_SHAPE
    inp = S.random_inputs(K, M, N, seed=9)
    ln = inp["lines"]
    us = []
    for rep in range(60):
        t0 = time.perf_counter()
        for k, kf in enumerate(inp["kfs"]):
            h, keep = kf_create(lib, kf)
            lib.ref_line_fuse_plain(h, M, _p(ln["start"]), _p(ln["end"]), _p(ln["normal"]), _p(ln["max_dist"]), _p(ln["desc"]),
                                    _p(np.ascontiguousarray(inp["skip"][k])), float(inp["th"]))
            lib.ref_line_kf_destroy(h)
        if rep >= 10:
            us.append((time.perf_counter() - t0) * 1e6)
    return dict(what=f"the reference's LineMatcher::Fuse as compiled by scripts/make_line_fuse_golden.py (-O2, no contraction), {K} calls: {K} key "
                     f"frames x {M} lines x {N} key lines (tests/line_fuse_scenario.random_inputs({K}, {M}, {N}, seed=9)), one core, wall "
                     "clock incl. filling the objects and the grid; median of 50 after 10",
                machine=f"{_cpu_model()}, {os.cpu_count()} logical CPUs (the host that ran this script, not the MI355X host of the GPU figures)",
                source="scripts/make_line_fuse_golden.py --time", us_median=round(float(np.median(us)), 1),
                us_p10=round(float(np.percentile(us, 10)), 1), us_p90=round(float(np.percentile(us, 90)), 1))


def main():
    with tempfile.TemporaryDirectory() as tmp:
        lib, overloads, defines = build_wrapper(tmp)
        inp, crowd = S.inputs(), S.crowd_inputs()
        counters, cc = {}, {}
        ld, ad = overloads["log"] != "std::log(float)", overloads["atan2"] != "atan2f"
        ref = compare(*ref_fuse(lib, inp), R.fuse_search(inp["kfs"], inp["lines"], inp["skip"], inp["th"], counters, ld, ad), inp["kfs"], "inputs")
        ref_c = compare(*ref_fuse(lib, crowd), R.fuse_search(crowd["kfs"], crowd["lines"], None, crowd["th"], cc, ld, ad), crowd["kfs"], "crowd")
        rnd = S.random_inputs(3, 120, 150, seed=3)
        compare(*ref_fuse(lib, rnd), R.fuse_search(rnd["kfs"], rnd["lines"], rnd["skip"], rnd["th"], None, ld, ad), rnd["kfs"], "random")
        # the ambiguous set: levels and thetas on both sides of a decision, where only the host's libm tells
        amb = S.ambiguous_inputs()
        ca = {}
        compare(*ref_fuse(lib, amb), R.fuse_search(amb["kfs"], amb["lines"], amb["skip"], amb["th"], ca, ld, ad), amb["kfs"], "ambiguous")
        assert ca["ambiguous_level"] >= 1 and ca["ambiguous_theta"] >= 1
        # GetLine2dRepresentation's theta alone against the restatement's call of the C library
        rng = np.random.default_rng(1)
        for xs, ys, xe, ye in rng.uniform(0, 640, (2000, 4)).astype(np.float32):
            nx, ny, _, _ = R.representation(xs, ys, xe, ye)
            assert np.float32(lib.ref_line_theta(float(xs), float(ys), float(xe), float(ye))).tobytes() == R.atan2_host(ny, nx, ad).tobytes()
        timing = time_reference(lib) if "--time" in sys.argv else None
    for k in R.REACHED + R.SUB_FACTS:
        if k in ("degenerate", "dist_zero", "end_points_coincide", "beyond_member_64"):
            assert counters[k] == 0, k            # undefined in the reference: not in its run; the crowd's own
            continue
        assert counters[k] >= 1, f"the reference's run does not take {k}: {counters}"
    assert cc["beyond_member_64"] >= 1 and cc["candidate"] == 8
    w = inp["where"]
    rk = lambda name, k=0: [int(ref["reached"][k, i]) for i in w[name]]
    expect = dict(candidate_mono=R.CANDIDATE, above_level=R.NO_CANDIDATE, below_level=R.NO_CANDIDATE, start_gate=R.NO_CANDIDATE,
                  end_gate=R.NO_CANDIDATE, right_gate=R.NO_CANDIDATE, u_right_start_zero=R.NO_CANDIDATE, u_right_end_negative=R.CANDIDATE,
                  dist_60=R.CANDIDATE, dist_61=R.ABOVE_TH_LOW, empty_window=R.EMPTY_WINDOW, clip_column_0=R.CANDIDATE, clip_column_159=R.CANDIDATE,
                  split_minus=R.CANDIDATE, split_plus_tie=R.CANDIDATE, middle_behind=R.MIDDLE_BEHIND, middle_outside=R.MIDDLE_OUTSIDE,
                  too_near=R.TOO_NEAR, too_far=R.TOO_FAR, end_behind=R.END_BEHIND, end_outside=R.END_OUTSIDE, view_angle=R.VIEW_ANGLE,
                  skip_null=R.SKIPPED, skip_bad=R.SKIPPED)
    for name, code in expect.items():
        assert all(r == code for r in rk(name)), f"{name}: the reference's run reached {rk(name)}, not {code}"
    assert rk("window_misses_grid", 2) == [R.EMPTY_WINDOW]
    assert rk("skip_in_kf", 1)[0] == R.SKIPPED and rk("skip_in_kf", 2)[1] == R.SKIPPED and rk("skip_in_kf", 0)[0] != R.SKIPPED
    assert [int(ref["n_proj"][0, i]) for i in w["end_outside"]] == [3, 2], "the two end points outside: the end's, then the start's"
    assert int(ref["raw_best_dist"][0, w["dist_60"][0]]) == 60 and int(ref["raw_best_dist"][0, w["dist_61"][0]]) == 61
    ja, jb = w["tie_indices"]
    assert ja > jb and int(ref["raw_best_idx"][0, w["split_plus_tie"][0]]) == ja, "the tie's winner is not the higher index"
    assert int(ref["raw_best_idx"][0, w["split_minus"][0]]) == w["split_minus_members"][0] and int(ref["n_dist"][0, w["split_minus"][0]]) == 2
    assert int(ref["n_dist"][0, w["split_plus_tie"][0]]) == 2
    facts = dict(counts=counters, crowd_counts=cc, ambiguous_counts={k: ca[k] for k in ("ambiguous_level", "ambiguous_theta")},
                 log_overload=overloads["log"], log_double_overload=int(ld), atan2_overload=overloads["atan2"], atan2_double_overload=int(ad),
                 defines=defines, n_fused=[int(n) for n in ref["n_fused"]], where={k: [int(i) for i in v] for k, v in w.items()})
    gdir = os.path.join(ROOT, "tests", "golden")
    digests = dict(inputs=S.digest(inp), crowd_inputs=S.digest(crowd))
    arrays = {k: v for k, v in ref.items()}
    arrays.update({"crowd_" + k: v for k, v in ref_c.items()})
    np.savez_compressed(os.path.join(gdir, "line_fuse_reference.npz"), **arrays, **{k + "_digest": np.array(v) for k, v in digests.items()})
    with open(os.path.join(gdir, "line_fuse_reference_facts.json"), "w") as fh:
        json.dump(dict(what="branch counts of the reference's LineMatcher::Fuse on tests/line_fuse_scenario.py (the restatement's counters, taken "
                            "only after the restatement reproduced the compiled cut bit for bit), the `log` and `atan2` overloads it was "
                            "compiled with (read off the compiled cut's undefined symbols), the #defines cut from src/LineMatcher.cc:38-40 "
                            "and src/MapLine.cc:33 — the replay rule of INTEGRATION.md 2j rests on USE_ENDPOINTS_AVERAGING == 0 — and the "
                            "placed cases (see scripts/make_line_fuse_golden.py)", digests=digests, facts=facts), fh, indent=1)
    if timing:
        tpath = os.path.join(ROOT, "profiles", "line_fuse_timing.json")
        doc = {}
        if os.path.exists(tpath):
            with open(tpath) as fh:
                doc = json.load(fh)
        doc["cpu_reference"] = timing
        with open(tpath, "w") as fh:
            json.dump(doc, fh, indent=1)
    print(json.dumps(facts)[:3000], timing)


if __name__ == "__main__":
    main()
