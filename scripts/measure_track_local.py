#!/usr/bin/env python3
"""Per-frame time of the local-map search on the GPU -> profiles/track_local_map_timing.json (beside the "cpu_reference" figure
scripts/make_track_local_golden.py measured on one core), at 3000 map points + 300 map lines over 1500 key points + 300 key lines
(tests/track_local_scenario.random_inputs()):
  --mode one_call     plvs_hip_frame_search_local_map: frustum loops and both searches, one wait                -> key "one_call"
  --mode two_entries  plvs_hip_orb_search_by_projection + plvs_hip_lines_search_by_projection fed precomputed frustum fields (the
                      numpy restatement's): what a caller can do without the one call, its host loop NOT counted -> key given by --key
                      (run with PLVS_HIP_LIB pointing at a build of the parent commit for "parent_two_entries")
  --mode stages       the one call's pieces: plvs_hip_frame_is_in_frustum alone, and the two entries as above   -> key "stages"
The C structures are built once; the clock is the host's around the raw ABI calls, which end in a stream wait.  Median of --calls
after --warmup."""
import argparse
import ctypes
import json
import os
import sys
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
    ap.add_argument("--mode", choices=("one_call", "two_entries", "stages"), required=True)
    ap.add_argument("--key", default="two_entries")
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "track_local_map_timing.json"))
    a = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "a measurement needs the GPU"
    from plvs_amd import _lib
    from tests import track_local_restatement as R
    from tests import track_local_scenario as S
    L, p = _lib.lib, _lib.np_ptr
    inp = S.random_inputs()
    m, ml, n, nl = len(inp["points"]["skip"]), len(inp["lines"]["skip"]), len(inp["frame"]["x"]), len(inp["frame"]["keylines"])
    fields = R.is_in_frustum(inp["cam"], inp["points"], inp["lines"])
    fv = S.frame_view(inp)
    fc = fv.as_c()
    lv, keep = S.line_view(inp)
    occ_p, occ_l = inp["frame"]["occupied_points"], inp["frame"]["occupied_lines"]
    ap_, al_ = np.zeros(n, np.int32), np.zeros(nl, np.int32)
    np_, nl_ = _i(), _i()
    mv = S.mappoint_view(inp["points"], fields)
    mc = mv.as_c()
    f_orb = L.plvs_hip_orb_search_by_projection
    f_orb.argtypes = [_vp, _vp, _f, _i, _f, _f, _vp, _vp, _vp]
    f_ln = L.plvs_hip_lines_search_by_projection
    f_ln.argtypes = [_vp, _vp, _i, _vp, _vp, _vp, _vp, _vp, _i, _f, _vp, _vp]
    l_in, l_proj, l_level = fields["l_in_view"], fields["l_proj"], fields["l_level"]
    ldesc, lobs = inp["lines"]["desc"], inp["lines"]["has_obs"]

    def two_entries():
        _lib.check(f_orb(ctypes.byref(fc), ctypes.byref(mc), 1.0, 0, 50.0, 0.8, p(occ_p), p(ap_), ctypes.byref(np_)))
        _lib.check(f_ln(ctypes.byref(lv), p(occ_l), ml, p(l_in), p(l_proj), p(l_level), p(ldesc), p(lobs), 0, 0.8, p(al_), ctypes.byref(nl_)))

    def clock(fn):
        t0 = time.perf_counter()
        fn()
        return (time.perf_counter() - t0) * 1e6

    def run(fn):
        return stats([clock(fn) for k in range(a.warmup + a.calls)][a.warmup:])

    workload = (f"{m} map points + {ml} map lines over {n} key points + {nl} key lines (tests/track_local_scenario.random_inputs()), "
                f"{fields['n_in_view_points']} points and {fields['n_in_view_lines']} lines in view, th 1, no far-point cut")
    if a.mode == "two_entries":
        result = dict(run(two_entries), library=os.path.basename(_lib.LIB_PATH), workload=workload + "; the two existing entries fed precomputed "
                      "frustum fields, two waits; the caller's host loop that makes the fields is not counted",
                      matches=[np_.value, nl_.value])
        key = a.key
    else:
        from plvs_amd import frame
        cc, k1 = frame._track_camera(inp["cam"])
        pc, k2, po = frame._track_points(inp["points"])
        lc, k3, lo = frame._track_lines(inp["lines"])
        nv, nvl, st = _i(), _i(), np.zeros(4, np.int32)

        def one_call():
            _lib.check(L.plvs_hip_frame_search_local_map(ctypes.byref(cc), ctypes.byref(fc), ctypes.byref(lv), ctypes.byref(pc), ctypes.byref(lc), 1.0, 0,
                                                         50.0, 0.8, 0, p(occ_p), p(occ_l), p(ap_), ctypes.byref(np_), p(al_), ctypes.byref(nl_),
                                                         ctypes.byref(nv), ctypes.byref(nvl), p(st), None))

        def frustum():
            _lib.check(L.plvs_hip_frame_is_in_frustum(ctypes.byref(cc), ctypes.byref(pc), ctypes.byref(lc), ctypes.byref(nv), ctypes.byref(nvl), p(st), None))

        if a.mode == "one_call":
            result = dict(run(one_call), workload=workload + "; frustum loops and both searches in one call",
                          matches=[np_.value, nl_.value], stats=[int(s) for s in st])
            two_entries()
            assert [np_.value, nl_.value] == result["matches"], "the one call and the two entries disagree"
            key = "one_call"
        else:
            result = dict(workload=workload, is_in_frustum=run(frustum), two_entries=run(two_entries), one_call=run(one_call))
            key = "stages"
    doc = {}
    if os.path.exists(a.out):
        with open(a.out) as fh:
            doc = json.load(fh)
    gpu = doc.setdefault("gpu", dict(what="per-call wall clock around the raw C ABI calls (ctypes, structures built once) on one MI355X; every call "
                                          "ends in a stream wait", source="scripts/measure_track_local.py"))
    gpu["device"] = torch.cuda.get_device_name(0)
    gpu[key] = result
    with open(a.out, "w") as fh:
        json.dump(doc, fh, indent=1)
    print(key, json.dumps(result))


if __name__ == "__main__":
    main()
