#!/usr/bin/env python3
"""Per-frame time of the motion-model search on the GPU -> profiles/track_motion_model_timing.json (beside the "cpu_reference" figure
scripts/make_track_motion_golden.py measured on one core), at 1500 last-frame points + 300 lines over 1500 key points + 300 key
lines (tests/track_motion_scenario.random_inputs()), th 15, orientation check on, both minima 0:
  --mode one_call     plvs_hip_frame_search_last_frame: projection and both searches, one wait                    -> key "one_call"
  --mode two_entries  plvs_hip_orb_search_by_projection_ff + plvs_hip_lines_search_by_projection_ff fed precomputed fields: what a
                      caller can do without the one call, its host loop NOT counted                               -> key given by --key
                      (run with PLVS_HIP_LIB pointing at a build of the parent commit for "parent_two_entries")
  --mode host_loop    that host loop alone: scripts/track_motion_host_loop.cpp, g++ -O2, no contraction, one core  -> key "host_loop"
Each mode is meant to run in a fresh process.  The C structures are built once; the clock is the host's around the raw ABI calls,
which end in a stream wait.  Median of --calls after --warmup, with p10 and p90."""
import argparse
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
_vp, _i, _f = ctypes.c_void_p, ctypes.c_int, ctypes.c_float


def stats(us):
    us = np.asarray(us)
    return dict(us_median=round(float(np.median(us)), 1), us_p10=round(float(np.percentile(us, 10)), 1),
                us_p90=round(float(np.percentile(us, 90)), 1), calls=int(len(us)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=("one_call", "two_entries", "host_loop"), required=True)
    ap.add_argument("--key", default="two_entries")
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "track_motion_model_timing.json"))
    a = ap.parse_args()
    from tests import track_motion_restatement as R
    from tests import track_motion_scenario as S
    inp = S.random_inputs()
    P, fr, pts, ln = inp["poses"], inp["frame"], inp["points"], inp["lines"]
    n, nl, N, NL = len(pts["valid"]), len(ln["valid"]), len(fr["x"]), len(fr["keylines"])
    fp, fl = R.project_points(P, pts), R.project_lines(P, ln)
    workload = (f"{n} last-frame points + {nl} lines over {N} key points + {NL} key lines (tests/track_motion_scenario.random_inputs()), "
                f"{int(fp['proj_valid'].sum())} points and {int(fl['proj_valid'].sum())} lines projected into the image, th 15, orientation check on")

    def clock(fn):
        t0 = time.perf_counter()
        fn()
        return (time.perf_counter() - t0) * 1e6

    def run(fn):
        return stats([clock(fn) for k in range(a.warmup + a.calls)][a.warmup:])

    device = None
    if a.mode == "host_loop":
        with tempfile.TemporaryDirectory() as tmp:
            so = os.path.join(tmp, "libhost_loop.so")
            subprocess.run(["g++", "-O2", "-std=c++14", "-fPIC", "-ffp-contract=off", "-fno-fast-math", "-shared",
                            os.path.join(ROOT, "scripts", "track_motion_host_loop.cpp"), "-o", so], check=True)
            lib = ctypes.CDLL(so)
        c = lambda x, t: np.ascontiguousarray(x, t)      # noqa: E731
        q, t, Rc, K, b = (c(P[k], np.float32) for k in ("q_cw", "tcw", "Rcw", "K4", "bounds4"))
        ins = [c(pts["valid"], np.uint8), c(pts["pos"], np.float32)]
        o = [np.zeros(n, np.uint8), np.zeros(n, np.float32), np.zeros(n, np.float32), np.zeros(n, np.float32)]
        lins = [c(ln["valid"], np.uint8), c(ln["start"], np.float32), c(ln["end"], np.float32), c(ln["max_dist"], np.float32)]
        lo = [np.zeros(nl, np.uint8), np.zeros((nl, 6), np.float32)]
        ptr = lambda x: x.ctypes.data_as(_vp)      # noqa: E731
        lib.host_loop.restype = None
        lib.host_loop.argtypes = [_vp] * 5 + [_i] + [_vp] * 6 + [_i] + [_vp] * 6
        args = [ptr(x) for x in (q, t, Rc, K, b)] + [n] + [ptr(x) for x in ins + o] + [nl] + [ptr(x) for x in lins + lo]
        result = dict(run(lambda: lib.host_loop(*args)), workload=workload + "; the projection loop alone, on the host, one core")
        for got, want in zip(o + lo, (fp["proj_valid"], fp["u"], fp["v"], fp["invz"], fl["proj_valid"], fl["proj6"])):
            assert got.tobytes() == np.ascontiguousarray(want).tobytes(), "the host loop and the restatement disagree"
        key = "host_loop"
    else:
        import torch
        assert torch.cuda.is_available(), "a measurement needs the GPU"
        device = torch.cuda.get_device_name(0)
        from plvs_amd import _lib
        from plvs_amd.orbmatcher import LastFrameView
        L, p = _lib.lib, _lib.np_ptr
        fv = S.frame_view(inp)
        fc = fv.as_c()
        lv, keep = S.line_view(inp)
        ang = np.ascontiguousarray(fr["cur_angle"], np.float32)
        occ_p, occ_l = fr["occupied_points"], fr["occupied_lines"]
        ap_, al_ = np.zeros(N, np.int32), np.zeros(NL, np.int32)
        np_, nl_ = _i(), _i()
        lf = LastFrameView(valid=fp["proj_valid"], u=fp["u"], v=fp["v"], invz=fp["invz"], octave=pts["octave"], angle=pts["angle"], desc=pts["desc"],
                           has_obs=pts["has_obs"])
        lfc = lf.as_c()
        f_orb = L.plvs_hip_orb_search_by_projection_ff
        f_orb.argtypes = [_vp, _vp, _f, _f, _f, _vp, _f, _i, _i, _i, _vp, _vp, _vp]
        f_ln = L.plvs_hip_lines_search_by_projection_ff
        f_ln.argtypes = [_vp, _vp, _i, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _f, _i, _vp, _vp]
        lvalid, proj6 = np.ascontiguousarray(fl["proj_valid"]), np.ascontiguousarray(fl["proj6"])
        loct, lang = np.ascontiguousarray(ln["octave"], np.int32), np.ascontiguousarray(ln["angle"], np.float32)

        def two_entries():
            _lib.check(f_orb(ctypes.byref(fc), p(ang), float(S.BOUNDS4[1]), float(S.BOUNDS4[3]), float(S.MBF), ctypes.byref(lfc), 15.0, 0, 0, 1, p(occ_p),
                             p(ap_), ctypes.byref(np_)))
            _lib.check(f_ln(ctypes.byref(lv), p(occ_l), nl, p(lvalid), p(proj6), p(loct), p(lang), p(ln["desc"]), p(ln["has_obs"]), 0, 0,
                            S.NN_RATIO_LINES, 1, p(al_), ctypes.byref(nl_)))

        if a.mode == "two_entries":
            result = dict(run(two_entries), library=os.path.basename(_lib.LIB_PATH), workload=workload + "; the two existing entries fed "
                          "precomputed fields, two waits; the caller's host loop that makes the fields is not counted", matches=[np_.value, nl_.value])
            key = a.key
        else:
            from plvs_amd import frame      # (not for a build of the parent commit: it lacks the entry)
            f32 = lambda x: np.ascontiguousarray(x, np.float32)      # noqa: E731
            keepp = [f32(P[k]) for k in ("q_cw", "tcw", "Rcw", "Ow", "q_lw", "tlw", "bounds4", "K4")]
            pc = frame.MotionPosesC(1, 0, 0, *[p(x) for x in keepp[:6]], float(P["mb"]), float(P["mbf"]), p(keepp[6]), p(keepp[7]), None)
            pin = [np.ascontiguousarray(pts["valid"], np.uint8), f32(pts["pos"]), np.ascontiguousarray(pts["octave"], np.int32), f32(pts["angle"]),
                   np.ascontiguousarray(pts["desc"]), np.ascontiguousarray(pts["has_obs"])]
            ptc = frame.MotionPointsC(n, *[p(x) for x in pin], None, None, None, None)
            lin = [np.ascontiguousarray(ln["valid"], np.uint8), f32(ln["start"]), f32(ln["end"]), f32(ln["max_dist"]), loct, lang,
                   np.ascontiguousarray(ln["desc"]), np.ascontiguousarray(ln["has_obs"])]
            lc = frame.MotionLinesC(nl, *[p(x) for x in lin], None, None)
            pol = frame.MotionPolicyC(15.0, 0.9, S.NN_RATIO_LINES, 1, 0, 0)
            res, st = frame.MotionResultC(), np.zeros(4, np.int32)

            def one_call():
                _lib.check(L.plvs_hip_frame_search_last_frame(ctypes.byref(pc), ctypes.byref(fc), p(ang), ctypes.byref(lv), ctypes.byref(ptc), ctypes.byref(lc),
                                                              ctypes.byref(pol), p(occ_p), p(occ_l), p(ap_), p(al_), ctypes.byref(res), p(st), None))

            result = dict(run(one_call), workload=workload + "; projection and both searches in one call", matches=[res.nmatches_points, res.nmatches_lines],
                          stats=[int(s) for s in st])
            two_entries()
            assert [np_.value, nl_.value] == result["matches"], "the one call and the two entries disagree"
            key = "one_call"
    doc = {}
    if os.path.exists(a.out):
        with open(a.out) as fh:
            doc = json.load(fh)
    if device is None:
        doc[key] = dict(result, source="scripts/measure_track_motion.py")
    else:
        gpu = doc.setdefault("gpu", dict(what="per-call wall clock around the raw C ABI calls (ctypes, structures built once) on one MI355X; every "
                                              "call ends in a stream wait", source="scripts/measure_track_motion.py"))
        gpu["device"] = device
        gpu[key] = result
    with open(a.out, "w") as fh:
        json.dump(doc, fh, indent=1)
    print(key, json.dumps(result))


if __name__ == "__main__":
    main()
