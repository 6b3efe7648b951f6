#!/usr/bin/env python3
"""Golden outputs of the REFERENCE'S OWN ORBmatcher::Fuse(pKF, vpMapPoints, th, bRight = false) on tests/orb_fuse_scenario.py.  The
definitions — ORBmatcher::Fuse (src/ORBmatcher.cc:1244-1434), KeyFrame::GetFeaturesInArea (src/KeyFrame.cc:1179-1229),
KeyFrame::IsInImage, MapPoint::PredictScale(const float&, KeyFramePtr&) (src/MapPoint.cc:581-596), Pinhole::project(const
Eigen::Vector3f&) and the three statements of Sophus' point action (so3.hpp:364-366) — are cut verbatim out of the reference tree
into a temporary directory at build time and compiled around scripts/ref_wrap/orb_fuse_ref_wrap.cpp (declarations, recording
accessors, calls and labelled restatements) against oracle/ref/eigen_full with -O2 -ffp-contract=off -fno-fast-math.  What each
pair did comes from the accessors the compiled text called.  Writes
  tests/golden/orb_fuse_reference.npz          reached, bestIdx, bestDist, distances taken, u, v per pair + the inputs digests
  tests/golden/orb_fuse_reference_facts.json   per-branch counts, the `log` overload compiled, the placed cases
and, with --time, the compiled cut's time on one core at 30 key frames x 1500 points x 1500 key points
(profiles/orb_fuse_timing.json, key "cpu_reference").  Dev-time tool: needs the reference tree.  Changes nothing under oracle/."""
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
from tests import orb_fuse_restatement as R                    # noqa: E402
from tests import orb_fuse_scenario as S                       # noqa: E402

_vp, _i, _f = ctypes.c_void_p, ctypes.c_int, ctypes.c_float
CUTS = {"orb_fuse_cut_defs.inc": (
            ("src/ORBmatcher.cc", r"/^    int ORBmatcher::Fuse\(KeyFramePtr& pKF, const vector<MapPointPtr> &vpMapPoints, const float th, const bool bRight\)/,/^    }/"),
            ("src/KeyFrame.cc", r"/^vector<size_t> KeyFrame::GetFeaturesInArea/,/^}/"),
            ("src/KeyFrame.cc", r"/^bool KeyFrame::IsInImage/,/^}/"),
            ("src/MapPoint.cc", r"/^int MapPoint::PredictScale\(const float &currentDist, KeyFramePtr& pKF\)/,/^}/"),
            ("src/CameraModels/Pinhole.cpp", r"/^    Eigen::Vector2f Pinhole::project\(const Eigen::Vector3f/,/^    }/")),
        "orb_fuse_cut_so3.inc": (("Thirdparty/Sophus/sophus/so3.hpp",
                                  r"/PointProduct<PointDerived> uv = q.vec\(\).cross\(p\);/,/return p \+ q.w\(\) \* uv \+ q.vec\(\).cross\(uv\);/"),)}
GOT_WORLD_POS, PROJECTED, GOT_MAX_DISTANCE, GOT_NORMAL, GOT_DESCRIPTOR, GOT_MAP_POINT, ADD_OBSERVATION, ADD_MAP_POINT, REPLACE = (1 << b for b in range(9))


def _p(a):
    return None if a is None else np.ascontiguousarray(a).ctypes.data_as(_vp)


def build_wrapper(tmp):
    ref, oref = reference_root(), os.path.join(ROOT, "oracle", "ref")
    for name, cuts in CUTS.items():
        with open(os.path.join(tmp, name), "w") as out:
            for path, pattern in cuts:
                text = subprocess.run(["awk", pattern, os.path.join(ref, path)], check=True, capture_output=True, text=True).stdout
                assert text.strip(), f"nothing cut from {path} by {pattern}"
                out.write(text + "\n")
    with open(os.path.join(tmp, "orb_fuse_cut_so3.inc")) as fh:
        assert len([ln for ln in fh.read().splitlines() if ln.strip()]) == 3, "the point action is no longer three statements"
    so = os.path.join(tmp, "liborb_fuse_ref.so")
    subprocess.run(["g++", "-O2", "-std=c++14", "-fPIC", "-ffp-contract=off", "-fno-fast-math", "-w", "-I" + os.path.join(oref, "eigen_full"),
                    "-I" + tmp, "-shared", os.path.join(ROOT, "scripts", "ref_wrap", "orb_fuse_ref_wrap.cpp"), "-o", so], check=True)
    undefined = subprocess.run(["nm", "-D", "--undefined-only", so], check=True, capture_output=True, text=True).stdout.split()
    names = {u.split("@")[0] for u in undefined}
    assert ("logf" in names) != ("log" in names), "the compiled PredictScale calls neither or both of logf / log"
    lib = ctypes.CDLL(so)
    lib.ref_kf_create.restype = _vp
    lib.ref_kf_create.argtypes = [_i] + [_vp] * 6 + [_f, _f, _vp, _f, _vp, _vp, _vp, _i, _vp, _vp, _f]
    lib.ref_kf_destroy.argtypes = [_vp]
    lib.ref_kf_destroy.restype = None
    lib.ref_fuse.restype = _i
    lib.ref_fuse.argtypes = [_vp, _i] + [_vp] * 6 + [_f, _vp, _vp, _vp]
    lib.ref_fuse_plain.restype = _i
    lib.ref_fuse_plain.argtypes = [_vp, _i] + [_vp] * 6 + [_f]
    lib.ref_predict_scale.restype = _i
    lib.ref_predict_scale.argtypes = [_f, _f, _f, _i]
    return lib, ("std::log(float)" if "logf" in names else "::log(double)")


def kf_create(lib, kf):
    keep = [np.ascontiguousarray(kf[k], t) for k, t in (("x", np.float32), ("y", np.float32), ("octave", np.int32), ("u_right", np.float32),
                                                       ("desc", np.uint8), ("bounds4", np.float32), ("K4", np.float32), ("q_cw", np.float32),
                                                       ("tcw", np.float32), ("Ow", np.float32), ("scale_factors", np.float32),
                                                       ("inv_level_sigma2", np.float32))]
    x, y, octv, ur, desc, b4, K4, q, t, Ow, sf, sig = keep
    assert (b4 == np.round(b4)).all() and b4[0] == kf["min_x"] and b4[2] == kf["min_y"], "the key frame holds its bounds as int"
    h = lib.ref_kf_create(len(x), _p(x), _p(y), _p(octv), _p(ur), _p(desc), _p(b4), float(kf["grid_w_inv"]), float(kf["grid_h_inv"]), _p(K4),
                          float(kf["mbf"]), _p(q), _p(t), _p(Ow), len(sf), _p(sf), _p(sig), float(kf["log_scale_factor"]))
    return h, keep


def ref_fuse(lib, inp):
    """The reference's Fuse, one call per key frame -> the restatement's fields as far as the accessors record them."""
    pts, K = inp["points"], len(inp["kfs"])
    M = len(pts["min_dist"])
    o = dict(reached=np.zeros((K, M), np.uint8), raw_best_idx=np.full((K, M), -1, np.int32), raw_best_dist=np.full((K, M), 256, np.int32),
             n_dist=np.zeros((K, M), np.int32), u=np.zeros((K, M), np.float32), v=np.zeros((K, M), np.float32), n_fused=np.zeros(K, np.int32))
    for k, kf in enumerate(inp["kfs"]):
        h, keep = kf_create(lib, kf)
        rec, uv, band = np.zeros((M, 4), np.int32), np.zeros((M, 2), np.float32), np.zeros(M, np.int32)
        sk = None if inp["skip"] is None else np.ascontiguousarray(inp["skip"][k])
        o["n_fused"][k] = lib.ref_fuse(h, M, _p(pts["pos"]), _p(pts["normal"]), _p(pts["min_dist"]), _p(pts["max_dist"]), _p(pts["desc"]), _p(sk),
                                       float(inp["th"]), _p(rec), _p(uv), _p(band))
        lib.ref_kf_destroy(h)
        for i in range(M):
            fl, nd, md, bi = (int(c) for c in rec[i])
            if not fl & GOT_WORLD_POS:
                r = R.SKIPPED
            elif not fl & PROJECTED:
                r = R.BEHIND
            elif not fl & GOT_MAX_DISTANCE:
                r = R.OUTSIDE
            elif not fl & GOT_NORMAL:
                assert band[i] in (1, 2), "stopped at the band, and neither comparison of :1323 holds"
                r = R.TOO_NEAR if band[i] == 1 else R.TOO_FAR
            elif not fl & GOT_DESCRIPTOR:
                # GetNormal, then no GetDescriptor: the viewing angle (:1331) or the empty window (:1344).  PredictScale and
                # GetFeaturesInArea are the cut's own and record nothing; the restatement, compared below, tells the two apart.
                r = None
            elif nd == 0:
                r = R.NO_CANDIDATE
            elif fl & GOT_MAP_POINT:
                assert fl & ADD_OBSERVATION and fl & ADD_MAP_POINT and not fl & REPLACE and md <= 50
                r = R.CANDIDATE
            else:
                assert md > 50
                r = R.ABOVE_TH_LOW
            o["reached"][k, i] = 255 if r is None else r
            o["n_dist"][k, i] = nd
            if fl & PROJECTED:
                o["u"][k, i], o["v"][k, i] = uv[i]
            if nd:
                o["raw_best_dist"][k, i] = md
            if fl & GOT_MAP_POINT:
                o["raw_best_idx"][k, i] = bi
        assert o["n_fused"][k] == int((o["reached"][k] == R.CANDIDATE).sum())
    return o


def same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def compare(ref, rest, name):
    """The restatement against the compiled cut, bit for bit.  A pair the accessors leave open (255) is the viewing angle or the
    empty window; bestIdx is observable where bestDist <= TH_LOW only."""
    open_ = ref["reached"] == 255
    assert np.isin(rest["reached"][open_], (R.VIEW_ANGLE, R.EMPTY_WINDOW)).all(), name
    assert same(np.where(open_, rest["reached"], ref["reached"]), rest["reached"]), f"{name}: reached differs at {np.argwhere(ref['reached'] != rest['reached'])[:8]}"
    for k in ("n_dist", "raw_best_dist", "u", "v"):
        assert same(ref[k], rest[k]), f"{name}: {k} differs at {np.argwhere(ref[k] != rest[k])[:8]}"
    assert same(ref["raw_best_idx"], rest["best_idx"]), f"{name}: bestIdx differs"
    out = dict(ref)
    out["reached"] = rest["reached"].copy()
    return out


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
    inp = S.random_inputs(30, 1500, 1500, seed=9)
    pts = inp["points"]
    M = len(pts["min_dist"])
    us = []
    for rep in range(12):
        t0 = time.perf_counter()
        for k, kf in enumerate(inp["kfs"]):
            h, keep = kf_create(lib, kf)
            lib.ref_fuse_plain(h, M, _p(pts["pos"]), _p(pts["normal"]), _p(pts["min_dist"]), _p(pts["max_dist"]), _p(pts["desc"]),
                               _p(np.ascontiguousarray(inp["skip"][k])), float(inp["th"]))
            lib.ref_kf_destroy(h)
        if rep >= 2:
            us.append((time.perf_counter() - t0) * 1e6)
    return dict(what="the reference's ORBmatcher::Fuse as compiled by scripts/make_orb_fuse_golden.py (-O2, no contraction), 30 calls: 30 key "
                     "frames x 1500 points x 1500 key points (tests/orb_fuse_scenario.random_inputs(30, 1500, 1500, seed=9)), one core, wall "
                     "clock incl. filling the objects and the grid; median of 10 after 2",
                machine=f"{_cpu_model()}, {os.cpu_count()} logical CPUs (the host that ran this script, not the MI355X host of the GPU figures)",
                source="scripts/make_orb_fuse_golden.py --time", us_median=round(float(np.median(us)), 1),
                us_p10=round(float(np.percentile(us, 10)), 1), us_p90=round(float(np.percentile(us, 90)), 1))


def main():
    with tempfile.TemporaryDirectory() as tmp:
        lib, overload = build_wrapper(tmp)
        inp, crowd = S.inputs(), S.crowd_inputs()
        counters, cc = {}, {}
        dbl = overload != "std::log(float)"
        ref = compare(ref_fuse(lib, inp), R.fuse_search(inp["kfs"], inp["points"], inp["skip"], inp["th"], counters, dbl), "inputs")
        ref_c = compare(ref_fuse(lib, crowd), R.fuse_search(crowd["kfs"], crowd["points"], None, crowd["th"], cc, dbl), "crowd")
        rnd = S.random_inputs(3, 120, 150, seed=3)
        compare(ref_fuse(lib, rnd), R.fuse_search(rnd["kfs"], rnd["points"], rnd["skip"], rnd["th"], None, dbl), "random")
        # PredictScale alone against the restatement's expression at ratios on both sides of an integer quotient
        amb = S.ambiguous_inputs()
        fr = R.front(amb["kfs"][0], amb["points"])
        levels = [lib.ref_predict_scale(float(fr["dist"][i]), float(amb["points"]["max_dist"][i]), float(S.LOG_SCALE), S.N_LEVELS) for i in range(24)]
        assert levels == [R.predict_scale(fr["ratio"][i], S.LOG_SCALE, S.N_LEVELS, dbl)[0] for i in range(24)]
        timing = time_reference(lib) if "--time" in sys.argv else None
    for k in R.REACHED + tuple(f for f in R.SUB_FACTS if f != "dist3d_zero"):
        assert counters[k] >= 1, f"the reference's run does not take {k}: {counters}"
    w = inp["where"]
    rk = lambda name, k=0: [int(ref["reached"][k, i]) for i in w[name]]
    expect = dict(candidate_mono=R.CANDIDATE, candidate_stereo=R.CANDIDATE, candidate_level_minus_1=R.CANDIDATE, below_level=R.NO_CANDIDATE,
                  above_level=R.NO_CANDIDATE, mono_gate=R.NO_CANDIDATE, stereo_gate=R.NO_CANDIDATE, u_right_zero=R.NO_CANDIDATE,
                  above_th_low=R.ABOVE_TH_LOW, tie=R.CANDIDATE, clip_left=R.CANDIDATE, clip_right=R.CANDIDATE, clip_top=R.CANDIDATE,
                  clip_bottom=R.CANDIDATE, empty_window=R.EMPTY_WINDOW, behind=R.BEHIND, outside=R.OUTSIDE, too_near=R.TOO_NEAR,
                  too_far=R.TOO_FAR, view_angle=R.VIEW_ANGLE, skip_null=R.SKIPPED, skip_bad=R.SKIPPED)
    for name, code in expect.items():
        assert all(r == code for r in rk(name)), f"{name}: the reference's run reached {rk(name)}, not {code}"
    assert rk("skip_in_kf", 0)[0] == R.SKIPPED and rk("skip_in_kf", 2)[1] == R.SKIPPED and rk("skip_in_kf", 1)[0] != R.SKIPPED
    ja, jb = w["tie_indices"]
    assert ja > jb and int(ref["raw_best_idx"][0, w["tie"][0]]) == ja, "the tie's winner is not the higher index"
    for name in ("z_zero_nan", "z_zero_inf"):
        i = w[name][0]
        assert ref["reached"][2, i] == R.OUTSIDE and not np.isfinite(ref["u"][2, i]), name
    assert np.isnan(ref["u"][2, w["z_zero_nan"][0]]) and np.isinf(ref["u"][2, w["z_zero_inf"][0]])
    assert cc["tie_winner_not_lowest_index"] >= 1 and cc["candidate"] == 8
    facts = dict(counts=counters, crowd_counts=cc, log_overload=overload, double_overload=int(dbl), n_fused=[int(n) for n in ref["n_fused"]],
                 where={k: [int(i) for i in v] for k, v in w.items()},
                 camera_centre_reached=[R.REACHED[int(ref["reached"][k, w["camera_centre"][0]])] for k in range(3)])
    gdir = os.path.join(ROOT, "tests", "golden")
    digests = dict(inputs=S.digest(inp), crowd_inputs=S.digest(crowd))
    arrays = {k: v for k, v in ref.items()}
    arrays.update({"crowd_" + k: v for k, v in ref_c.items()})
    np.savez_compressed(os.path.join(gdir, "orb_fuse_reference.npz"), **arrays, **{k + "_digest": np.array(v) for k, v in digests.items()})
    with open(os.path.join(gdir, "orb_fuse_reference_facts.json"), "w") as fh:
        json.dump(dict(what="branch counts of the reference's ORBmatcher::Fuse on tests/orb_fuse_scenario.py (the restatement's counters, taken "
                            "only after the restatement reproduced the compiled cut bit for bit), the `log` overload its PredictScale was "
                            "compiled with and the placed cases (see scripts/make_orb_fuse_golden.py)", digests=digests, facts=facts), fh, indent=1)
    if timing:
        tpath = os.path.join(ROOT, "profiles", "orb_fuse_timing.json")
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
