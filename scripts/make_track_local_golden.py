#!/usr/bin/env python3
"""Golden outputs of the REFERENCE'S OWN Frame::isInFrustum(MapPointPtr&, float) / (MapLinePtr&, float) on
tests/track_local_scenario.py, and of the reference's two local-map searches on the fields it leaves.  The definitions — the two
isInFrustum, MapPoint / MapLine::PredictScale(const float&, Frame*), the four Get{Min,Max}DistanceInvariance and
Pinhole::project(const Eigen::Vector3f&) — are cut verbatim out of the reference tree into a temporary directory at build time
and compiled around scripts/ref_wrap/track_local_ref_wrap.cpp (declarations and calls only) against oracle/ref/eigen_full with
-O2 -ffp-contract=off -fno-fast-math; the searches come from oracle/_ref/libmatchers_ref.so as it is.  Writes
  tests/golden/track_local_reference.npz          every output array of the reference's runs + the inputs digests
  tests/golden/track_local_reference_facts.json   per-branch counts (the restatement's counters, taken only after the restatement
                                                  has reproduced the reference bit for bit) and the `log` overload compiled
and asserts ON THE REFERENCE'S RUN that the scenario takes every branch it was built for.  It also times the reference's two loops
plus two searches on one core at 3000 points + 300 lines (profiles/track_local_map_timing.json, key "cpu_reference").  Dev-time
tool: needs the reference tree and the compiled reference library.  Changes nothing under oracle/."""
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
from tests import track_local_restatement as R                 # noqa: E402
from tests import track_local_scenario as S                    # noqa: E402

_vp, _i, _f = ctypes.c_void_p, ctypes.c_int, ctypes.c_float
CUTS = (("src/Frame.cc", r"/^bool Frame::isInFrustum\(MapPointPtr/,/^}/"),
        ("src/Frame.cc", r"/^bool Frame::isInFrustum\(MapLinePtr/,/^}/"),
        ("src/MapPoint.cc", r"/^int MapPoint::PredictScale\(const float &currentDist, Frame/,/^}/"),
        ("src/MapLine.cc", r"/^int MapLine::PredictScale\(const float &currentDist, Frame/,/^}/"),
        ("src/MapPoint.cc", r"/^float MapPoint::GetMinDistanceInvariance/,/^}/"),
        ("src/MapPoint.cc", r"/^float MapPoint::GetMaxDistanceInvariance/,/^}/"),
        ("src/MapLine.cc", r"/^float MapLine::GetMinDistanceInvariance/,/^}/"),
        ("src/MapLine.cc", r"/^float MapLine::GetMaxDistanceInvariance/,/^}/"),
        ("src/CameraModels/Pinhole.cpp", r"/^    Eigen::Vector2f Pinhole::project\(const Eigen::Vector3f/,/^    }/"))
POINT_REACHED = ("skipped", "behind", "pcz_zero", "out_left", "out_right", "out_top", "out_bottom", "too_near", "too_far", "grazing", "in_view",
                 "level_at_0", "level_above_top", "view_cos_above_998", "view_cos_below_998")
# nScale < 0 needs ratio < 1 / 1.2 while the distance band admits dist <= 1.2f * mfMaxDistance only: the lower clamp is reached as
# nScale == 0 (level_at_0), the branch nScale < 0 by no input that passes the band
UNREACHABLE = ("level_below_0",)
LINE_REACHED = ("skipped", "behind", "out_left", "out_right", "out_top", "out_bottom", "too_near", "near_quirk", "too_far", "grazing", "in_view",
                "end_behind")


def _p(a):
    return None if a is None else np.ascontiguousarray(a).ctypes.data_as(_vp)


def build_wrapper(tmp):
    ref, oref = reference_root(), os.path.join(ROOT, "oracle", "ref")
    with open(os.path.join(tmp, "track_local_cut.inc"), "w") as out:
        for path, pattern in CUTS:
            text = subprocess.run(["awk", pattern, os.path.join(ref, path)], check=True, capture_output=True, text=True).stdout
            assert text.strip(), f"nothing cut from {path} by {pattern}"
            out.write(text + "\n")
    so = os.path.join(tmp, "libtrack_local_ref.so")
    subprocess.run(["g++", "-O2", "-std=c++14", "-fPIC", "-ffp-contract=off", "-fno-fast-math", "-w", "-I" + os.path.join(oref, "eigen_full"),
                    "-I" + tmp, "-shared", os.path.join(ROOT, "scripts", "ref_wrap", "track_local_ref_wrap.cpp"), "-o", so], check=True)
    undefined = subprocess.run(["nm", "-D", "--undefined-only", so], check=True, capture_output=True, text=True).stdout.split()
    names = {u.split("@")[0] for u in undefined}
    assert ("logf" in names) != ("log" in names), "the compiled PredictScale calls neither or both of logf / log"
    return ctypes.CDLL(so), ("std::log(float)" if "logf" in names else "::log(double)")


def ref_frustum(lib, cam, points, lines):
    """The reference's two loops -> the output arrays under the restatement's names."""
    out = {}
    c = [np.ascontiguousarray(cam[k], np.float32) for k in ("K4", "bounds4", "Rcw", "tcw", "Ow")]
    if points is not None:
        m = len(points["skip"])
        o = dict(in_view=np.zeros(m, np.uint8), proj_x=np.full(m, -1, np.float32), proj_y=np.full(m, -1, np.float32), proj_xr=np.zeros(m, np.float32),
                 track_depth=np.zeros(m, np.float32), level=np.zeros(m, np.int32), view_cos=np.zeros(m, np.float32))
        fn = lib.ref_is_in_frustum_points
        fn.restype = _i
        fn.argtypes = [_vp, _f, _vp, _vp, _vp, _vp, _f, _f, _i, _i] + [_vp] * 12
        n = fn(_p(c[0]), float(cam["mbf"]), _p(c[1]), _p(c[2]), _p(c[3]), _p(c[4]), float(cam["viewing_cos_limit"]), float(cam["log_scale_factor"]),
               cam["n_levels"], m, _p(points["skip"]), _p(points["pos"]), _p(points["normal"]), _p(points["min_dist"]), _p(points["max_dist"]),
               *[_p(o[k]) for k in ("in_view", "proj_x", "proj_y", "proj_xr", "track_depth", "level", "view_cos")])
        # the fields the reference leaves stale on a point it rejects are reported as 0 (include/plvs_hip.h)
        rej = o["in_view"] == 0
        for k in ("proj_xr", "track_depth", "view_cos"):
            o[k][rej] = 0
        o["level"][rej] = 0
        out.update({"p_" + k: v for k, v in o.items()})
        out["n_in_view_points"] = n
    if lines is not None:
        m = len(lines["skip"])
        proj = np.zeros((m, 6), np.float32)
        proj[:, :4] = -1
        o = dict(in_view=np.zeros(m, np.uint8), proj=proj, proj_xr=np.full((m, 2), -1, np.float32), level=np.zeros(m, np.int32),
                 view_cos=np.zeros(m, np.float32))
        fn = lib.ref_is_in_frustum_lines
        fn.restype = _i
        fn.argtypes = [_vp, _f, _vp, _vp, _vp, _vp, _f, _f, _i, _i] + [_vp] * 10
        n = fn(_p(c[0]), float(cam["mbf"]), _p(c[1]), _p(c[2]), _p(c[3]), _p(c[4]), float(cam["viewing_cos_limit"]),
               float(cam["line_log_scale_factor"]), cam["n_line_levels"], m, _p(lines["skip"]), _p(lines["start"]), _p(lines["end"]),
               _p(lines["normal"]), _p(lines["max_dist"]), *[_p(o[k]) for k in ("in_view", "proj", "proj_xr", "level", "view_cos")])
        out.update({"l_" + k: v for k, v in o.items()})
        out["n_in_view_lines"] = n
    return out


def ref_point_search(mlib, inp, fields, th, far, occ, th_far=float(S.TH_FAR)):
    fc, mc = S.frame_view(inp).as_c(), S.mappoint_view(inp["points"], fields).as_c()
    a = np.full(fc.n, -7, np.int32)
    fn = mlib.ref_orb_search_by_projection
    fn.argtypes = [_vp, _vp, _f, _i, _f, _f, _vp, _vp]
    fn.restype = _i
    n = fn(ctypes.byref(fc), ctypes.byref(mc), th, int(far), th_far, S.NN_RATIO, _p(inp["frame"]["occupied_points"]) if occ else None, _p(a))
    return n, a


def ref_line_search(mlib, inp, fields, larger, occ):
    F, keep = S.line_view(inp)
    a = np.full(F.n, -7, np.int32)
    fn = mlib.ref_lines_search_by_projection
    fn.restype = _i
    fn.argtypes = [_vp, _vp, _i, _vp, _vp, _vp, _vp, _vp, _i, _f, _vp]
    L = inp["lines"]
    n = fn(ctypes.byref(F), _p(inp["frame"]["occupied_lines"]) if occ else None, len(L["skip"]), _p(fields["l_in_view"]), _p(fields["l_proj"]),
           _p(fields["l_level"]), _p(L["desc"]), _p(L["has_obs"]), int(larger), S.NN_RATIO, _p(a))
    return n, a


def same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def compare(ref, rest):
    for k, v in ref.items():
        if isinstance(v, np.ndarray):
            assert same(v, rest[k]), f"the restatement differs from the reference in {k}: {np.flatnonzero((v != rest[k]).reshape(len(v), -1).any(1))[:8]}"
        else:
            assert v == rest[k], k


def time_reference(lib, mlib):
    inp = S.random_inputs()
    us = []
    for k in range(60):
        t0 = time.perf_counter()
        f = ref_frustum(lib, inp["cam"], inp["points"], inp["lines"])
        ref_point_search(mlib, inp, f, 1.0, False, True)
        ref_line_search(mlib, inp, f, False, True)
        if k >= 10:
            us.append((time.perf_counter() - t0) * 1e6)
    return dict(what="the reference's Frame::isInFrustum over 3000 map points + 300 map lines and its two SearchByProjection (the cut definitions and "
                     "oracle/_ref/libmatchers_ref.so: -O2, no contraction), one core, tests/track_local_scenario.random_inputs(), wall clock per "
                     "frame incl. filling the objects; median of 50 after 10",
                source="scripts/make_track_local_golden.py", us_median=round(float(np.median(us)), 1), us_p10=round(float(np.percentile(us, 10)), 1),
                us_p90=round(float(np.percentile(us, 90)), 1))


def main():
    inp, crowd = S.inputs(), S.crowd_inputs()
    mlib = ctypes.CDLL(os.path.join(ROOT, "oracle", "_ref", "libmatchers_ref.so"))
    with tempfile.TemporaryDirectory() as tmp:
        lib, overload = build_wrapper(tmp)
        ref = ref_frustum(lib, inp["cam"], inp["points"], inp["lines"])
        ref_c = ref_frustum(lib, crowd["cam"], crowd["points"], None)
        # PredictScale alone, for both kinds, against the restatement's expression at the placed ratios
        lib.ref_predict_scale.restype = _i
        lib.ref_predict_scale.argtypes = [_i, _f, _f, _f, _i]
        timing = time_reference(lib, mlib)
        counters = {}
        rest = R.is_in_frustum(inp["cam"], inp["points"], inp["lines"], counters=counters)
        compare(ref, rest)
        compare(ref_c, R.is_in_frustum(crowd["cam"], crowd["points"], None))
        for kind, key, levels in ((0, "p_", S.N_LEVELS), (1, "l_", S.N_LINE_LEVELS)):
            for k in np.flatnonzero(rest[key + "in_view"]):
                r = rest[key + "ratio"][k]
                assert lib.ref_predict_scale(kind, float(r), 1.0, float(S.LOG_SCALE), levels) == rest[key + "level"][k]
    cp, cl = counters["points"], counters["lines"]
    for k in POINT_REACHED:
        assert cp[k] >= 1, f"the reference's run over the points does not take the branch {k}"
    for k in LINE_REACHED:
        assert cl[k] >= 1, f"the reference's run over the lines does not take the branch {k}"
    for k in UNREACHABLE:
        assert cp[k] == 0 and cl[k] == 0, k
    w = inp["where"]
    # the placed cases, read back from the reference's outputs
    for k in ("behind", "out_left", "out_right", "out_top", "out_bottom", "pcz_zero"):
        assert all(ref["p_in_view"][i] == 0 and ref["p_proj_x"][i] == -1 for i in w[k]), k
    for k in ("too_near", "too_far", "grazing_rejected"):
        assert all(ref["p_in_view"][i] == 0 and ref["p_proj_x"][i] != -1 for i in w[k]), k
    for k in ("grazing_kept", "view_cos_above_998", "view_cos_below_998", "far_cut", "level_clamped_0", "level_clamped_top"):
        assert all(ref["p_in_view"][i] == 1 for i in w[k]), k
    assert all(ref["p_view_cos"][i] > 0.998 for i in w["view_cos_above_998"]) and all(ref["p_view_cos"][i] <= 0.998 for i in w["view_cos_below_998"])
    assert all(ref["p_track_depth"][i] > S.TH_FAR for i in w["far_cut"])
    assert all(ref["p_level"][i] == 0 for i in w["level_clamped_0"]) and all(ref["p_level"][i] == S.N_LEVELS - 1 for i in w["level_clamped_top"])
    assert all(ref["l_in_view"][i] == 0 for k in ("line_near_quirk", "line_too_far", "line_grazing_rejected", "line_behind", "line_outside") for i in w[k])
    assert all(ref["l_in_view"][i] == 1 for k in ("line_grazing_kept", "line_end_behind") for i in w[k])
    i = w["line_end_behind"][0]
    assert ref["l_proj"][i, 5] < 0 < ref["l_proj"][i, 4]
    assert cl["near_quirk"] >= len(w["line_near_quirk"])
    # the placed ratios: marked ambiguous, in view, and the levels on both sides of the integer occur
    sides_p = {(k, int(ref["p_level"][i]) - k) for i, k, _ in w["ratio_points"]}
    sides_l = {(k, int(ref["l_level"][i]) - k) for i, k, _ in w["ratio_lines"]}
    assert all(rest["p_ambiguous"][i] and ref["p_in_view"][i] for i, _, _ in w["ratio_points"]), "a placed point ratio is not marked"
    assert all(rest["l_ambiguous"][i] and ref["l_in_view"][i] for i, _, _ in w["ratio_lines"]), "a placed line ratio is not marked"
    assert {d for _, d in sides_p} == {0, 1} and {d for k, d in sides_l if k == 1} == {0, 1}, (sides_p, sides_l)
    assert cp["ambiguous"] >= 6 and cl["ambiguous"] >= 2 and cp["ambiguous"] + cl["ambiguous"] >= 8
    both = {"std::log(float)": False, "::log(double)": True}
    differ = [int(i) for i, _, _ in w["ratio_points"]
              if R.predict_scale(rest["p_ratio"][i], S.LOG_SCALE, S.N_LEVELS, False)[0] != R.predict_scale(rest["p_ratio"][i], S.LOG_SCALE, S.N_LEVELS, True)[0]]
    # ---- the searches on the reference's fields
    arrays = {k: v for k, v in ref.items() if isinstance(v, np.ndarray)}
    arrays.update({"crowd_" + k: v for k, v in ref_c.items() if isinstance(v, np.ndarray)})
    searches = {}
    for th, far, occ in S.SEARCH_CASES:
        n, a = ref_point_search(mlib, inp, ref, th, far, occ)
        arrays[S.search_key(th, far, occ)] = a
        searches[S.search_key(th, far, occ)] = n
    assert len({arrays[S.search_key(th, far, True)].tobytes() for th in (1.0, 3.0, 15.0) for far in (False, True)}) == 6, "th / far do not bite"
    assert searches[S.search_key(1.0, False, True)] > 150
    for larger, occ in S.LINE_CASES:
        n, a = ref_line_search(mlib, inp, ref, larger, occ)
        arrays[S.line_key(larger, occ)] = a
        searches[S.line_key(larger, occ)] = n
    assert searches[S.line_key(False, True)] > 30
    n, a = ref_point_search(mlib, crowd, ref_c, 1.0, False, True)
    arrays["crowd_assigned_points"] = a
    searches["crowd_assigned_points"] = n
    facts = dict(points=cp, lines=cl, n_in_view_points=ref["n_in_view_points"], n_in_view_lines=ref["n_in_view_lines"],
                 crowd_n_in_view_points=ref_c["n_in_view_points"], log_overload=overload, double_overload=both[overload],
                 ratio_points_where_the_two_overloads_differ=differ, nmatches=searches,
                 ratio_points=[[int(i), int(k), int(o), int(ref["p_level"][i])] for i, k, o in w["ratio_points"]],
                 ratio_lines=[[int(i), int(k), int(o), int(ref["l_level"][i])] for i, k, o in w["ratio_lines"]])
    gdir = os.path.join(ROOT, "tests", "golden")
    np.savez_compressed(os.path.join(gdir, "track_local_reference.npz"), **arrays, inputs_digest=np.array(S.inputs_digest(inp)),
                        crowd_inputs_digest=np.array(S.inputs_digest(crowd)))
    with open(os.path.join(gdir, "track_local_reference_facts.json"), "w") as fh:
        json.dump(dict(what="branch counts of the reference's Frame::isInFrustum loops on tests/track_local_scenario.py, the `log` overload its "
                            "PredictScale was compiled with, and the return values of its two searches (see scripts/make_track_local_golden.py)",
                       inputs=S.inputs_digest(inp), crowd_inputs=S.inputs_digest(crowd), facts=facts), fh, indent=1)
    tpath = os.path.join(ROOT, "profiles", "track_local_map_timing.json")
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
