#!/usr/bin/env python3
"""Per-call time of the loop-closing SearchByProjection searches over resident key frames -> profiles/loop_search_timing.json.

Shapes (chosen ones: the reference's sizes depend on the data), th 3, ratio 1.5 as src/LoopClosing.cc:1237/1245 call them:
  K1   1 key frame x 5 000 map points x 1 500 key points, and x 1 000 map lines x 300 key lines;
  K5   5 key frames of the same (tests/loop_search_scenario.nominal_point_inputs / nominal_line_inputs: the verification loop of
       :1021-1044 — covisible key frames a few centimetres and degrees apart, the points back-projections of their key points).
Figures per shape: the point entry, the line entry, both kinds in one call; K calls of one key frame each in a row (what a caller
without the batch pays); the two host twins.  One set of handles and ONE pose list serves every figure of a shape (the handles' own:
the line set's matrix and translation with the point set's quaternion; both sets are generated from the same poses).  The clock is
the host's around the raw ABI calls, which end in a stream wait and the greedy pass; the C structures and the handles are made
before it starts.  The device figures run in --rounds rounds, alternating between the entries, median of --calls after --warmup with
p10 and p90 per round.  scripts/make_loop_search_golden.py --time adds "cpu_reference" (the compiled reference cuts, one core) to
the same file.  No threshold is asserted anywhere; bench.py does not call these entries."""
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
SHAPES = dict(K1=1, K5=5)
TH, RATIO = 3.0, 1.5


def stats(us):
    us = np.asarray(us)
    return dict(us_median=round(float(np.median(us)), 1), us_p10=round(float(np.percentile(us, 10)), 1),
                us_p90=round(float(np.percentile(us, 90)), 1), calls=int(len(us)))


def timed(call, calls, warmup):
    from plvs_amd import _lib
    us = []
    for _ in range(warmup + calls):
        t0 = time.perf_counter()
        rc = call()
        us.append((time.perf_counter() - t0) * 1e6)
        _lib.check(rc)
    return stats(us[warmup:])


def shape_figures(K, a):
    from plvs_amd import _lib
    from plvs_amd.keyframe import _lists
    from tests import loop_search_scenario as S
    import torch
    assert torch.cuda.is_available(), "a measurement needs the GPU"
    L, p = _lib.lib, _lib.np_ptr
    pin, lin = S.nominal_point_inputs(K), S.nominal_line_inputs(K)
    out = dict(shape=dict(points="%d key frames x %d map points x %d key points" % (K, len(pin["points"]["min_dist"]), len(pin["kfs"][0]["x"])),
                          lines="%d key frames x %d map lines x %d key lines" % (K, len(lin["lines"]["max_dist"]), len(lin["kfs"][0]["kl"]))),
               th=TH, ratio_hamming=RATIO, device=torch.cuda.get_device_name(0))
    mk = lambda k, m: (np.zeros((k, m), np.int32), np.zeros((k, m), np.int32), np.zeros((k, m), np.uint8), np.zeros(k, np.int32), np.zeros(5, np.int32))
    ptrs = lambda o: [p(x) for x in o]
    with S.Handles(points_inp=pin, lines_inp=lin) as h:
        _, hs, ps = _lists(h.kfs, h.poses)
        pc, lc = h.points.as_c(), h.lines.as_c()
        psk, lsk = np.ascontiguousarray(pin["skip"], np.uint8), np.ascontiguousarray(lin["skip"], np.uint8)
        po, lo, st = mk(K, pc.m), mk(K, lc.m), np.zeros(3, np.int32)
        fp_, fl_ = L.plvs_hip_orb_loop_search_by_projection_kf, L.plvs_hip_line_loop_search_by_projection_kf
        fp_.argtypes = [_vp, _vp, _i, _vp, _vp, _vp, _f, _f, _i] + [_vp] * 6
        fl_.argtypes = [_vp, _vp, _i, _vp, _vp, _vp, _f, _f] + [_vp] * 6
        both = L.plvs_hip_loop_search_by_projection_points_and_lines_kf
        both.argtypes = [_vp, _vp, _i, _vp, _vp, _vp, _f, _f, _i] + [_vp] * 5 + [_vp, _vp, _vp, _f, _f] + [_vp] * 5 + [_vp, _vp]
        calls = dict(points=lambda: fp_(hs, ps, K, ctypes.byref(pc), p(psk), None, TH, RATIO, 0, *ptrs(po), None),
                     lines=lambda: fl_(hs, ps, K, ctypes.byref(lc), p(lsk), None, TH, RATIO, *ptrs(lo), None),
                     both=lambda: both(hs, ps, K, ctypes.byref(pc), p(psk), None, TH, RATIO, 0, *ptrs(po), ctypes.byref(lc), p(lsk), None, TH, RATIO,
                                       *ptrs(lo), p(st), None))
        # one key frame per call, K calls in a row, points then lines each time (as the reference's loop runs them)
        hk = [(_vp * 1)(h.kfs[k].handle) for k in range(K)]
        pk = [_lists([h.kfs[k]], [h.poses[k]])[2] for k in range(K)]
        prow, lrow = [np.ascontiguousarray(psk[k:k + 1]) for k in range(K)], [np.ascontiguousarray(lsk[k:k + 1]) for k in range(K)]
        po1, lo1 = mk(1, pc.m), mk(1, lc.m)

        def single_calls():
            for k in range(K):
                rc = fp_(hk[k], pk[k], 1, ctypes.byref(pc), p(prow[k]), None, TH, RATIO, 0, *ptrs(po1), None)
                rc = rc or fl_(hk[k], pk[k], 1, ctypes.byref(lc), p(lrow[k]), None, TH, RATIO, *ptrs(lo1), None)
                if rc:
                    return rc
            return 0
        calls["single_key_frame_calls"] = single_calls
        rounds = {k: [] for k in calls}
        for _ in range(a.rounds):
            for key, call in calls.items():
                rounds[key].append(timed(call, a.calls, a.warmup))
        med = lambda key: round(float(np.median([r["us_median"] for r in rounds[key]])), 1)
        out["rounds"] = rounds
        out["us_median_of_rounds"] = {k: med(k) for k in calls}
        out["what"] = dict(points="plvs_hip_orb_loop_search_by_projection_kf (PLVS_LOOP_PROJECT_CAMERA)", lines="plvs_hip_line_loop_search_by_projection_kf",
                           both="plvs_hip_loop_search_by_projection_points_and_lines_kf: one copy in, two launches, one wait, two greedy passes",
                           single_key_frame_calls=f"{K} x (one point call + one line call) of one key frame each, in a row")
        calls["points"]()
        calls["lines"]()
        for kind, o, first, cand in (("points", po, 6, 9), ("lines", lo, 9, 12)):
            reached = o[2]
            out[kind + "_result"] = dict(stats=o[4].tolist(), nmatches=o[3].tolist(), pairs=int(reached.size),
                                         survivor_fraction=round(float((reached >= first).sum()) / max(int((reached != 0).sum()), 1), 4),
                                         matched=int((reached == cand).sum()))
        calls["both"]()
        out["both_call_stats"] = st.tolist()
        fph, flh = L.plvs_hip_orb_loop_search_by_projection_kf_host, L.plvs_hip_line_loop_search_by_projection_kf_host
        fph.argtypes, flh.argtypes = fp_.argtypes[:-1], fl_.argtypes[:-1]
        dev = [x.copy() for x in po[:4]] + [x.copy() for x in lo[:4]]
        out["points_host"] = dict(timed(lambda: fph(hs, ps, K, ctypes.byref(pc), p(psk), None, TH, RATIO, 0, *ptrs(po)), 5, 1),
                                  what="plvs_hip_orb_loop_search_by_projection_kf_host, serial, on the handles' host copies")
        out["lines_host"] = dict(timed(lambda: flh(hs, ps, K, ctypes.byref(lc), p(lsk), None, TH, RATIO, *ptrs(lo)), 5, 1),
                                 what="plvs_hip_line_loop_search_by_projection_kf_host")
        assert all((x == y).all() for x, y in zip(dev, list(po[:4]) + list(lo[:4]))), "the device entries and the host twins disagree"
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="K1,K5")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--calls", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "loop_search_timing.json"))
    a = ap.parse_args()
    doc = {}
    if os.path.exists(a.out):
        with open(a.out) as fh:
            doc = json.load(fh)
    doc.update(what="per-call wall clock around the raw C ABI calls (ctypes, structures and handles built once) on one MI355X; every device "
                    "call ends in a stream wait and the host's greedy pass; the entries run alternately in rounds in one process; bench.py does "
                    "not call these entries",
               source="scripts/measure_loop_search.py")
    for name in a.shapes.split(","):
        doc[name] = shape_figures(SHAPES[name], a)
        print(name, json.dumps(doc[name]["us_median_of_rounds"]), json.dumps(doc[name]["points_host"]), json.dumps(doc[name]["lines_host"]), flush=True)
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(doc, fh, indent=1)


if __name__ == "__main__":
    main()
