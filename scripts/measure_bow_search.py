#!/usr/bin/env python3
"""Per-call time of ORBmatcher::SearchByBoW over resident key frames -> profiles/bow_search_timing.json.

Shapes (tests/bow_search_scenario.nominal: chosen ones, the reference's sizes depend on the data):
  loop_detection   SearchByBoW(pKF1, pKF2[k]) for 33 key frames of 1 500 key points, about 100 vocabulary nodes, ratio 0.9
                   (src/LoopClosing.cc:769-780: 11 calls per candidate, three candidates)
  relocalisation   SearchByBoW(pKF[k], F) for 10 candidates against a frame of 1 500 key points, ratio 0.75 (src/Tracking.cc:4907-4930)
Figures per shape: the one-call entry; K calls of the one-call entry with one key frame each; K calls of plvs_hip_orb_search_by_bow
(every call uploads both descriptor sets and the pair lists, the greedy pass on the host) — for the key-frame kind the caller passes
KF2 as the "frame", the nearest thing that entry offers: ITS SEMANTICS DIFFER (no validity gate on KF2, <= TH_LOW), so this is a cost
comparison alone; the host twin.  The clock is the host's around the raw ABI calls, which end in a stream wait and the host's
histogram pass; the C structures and the handles are made before it starts.  The device figures run in --rounds rounds, alternating
between the entries, median of --calls after --warmup with p10 and p90 per round.  scripts/make_bow_search_golden.py --time adds
"cpu_reference" (the compiled reference cuts, one core) to the same file.  No threshold is asserted; bench.py does not call these entries."""
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
SHAPES = dict(loop_detection=("kf", 33, 0.9), relocalisation=("frame", 10, 0.75))


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


def shape_figures(kind, K, ratio, a):
    from plvs_amd import _lib
    from tests import bow_search_scenario as S
    import torch
    assert torch.cuda.is_available(), "a measurement needs the GPU"
    L, p = _lib.lib, _lib.np_ptr
    a_side, b_sides = S.nominal(K)
    n = len(a_side["desc"])
    out = dict(shape="%d key frames of %d key points against one of %d, %d vocabulary nodes" % (K, len(b_sides[0]["desc"]), n, len(a_side["nodes"])),
               kind=kind, nn_ratio=ratio, check_orientation=1, device=torch.cuda.get_device_name(0))
    ha = S.key_frame(a_side)
    hb = [S.key_frame(b) for b in b_sides]
    try:
        va, vb = S.valid_of(a_side), [S.valid_of(b) for b in b_sides]
        hs = (_vp * K)(*[h.handle for h in hb])
        vs = (_vp * K)(*[v.ctypes.data for v in vb])
        frame = S.bow_frame(a_side)
        fc = frame.as_c()
        mk = lambda k: (np.zeros((k, n), np.int32), np.zeros((k, n), np.int32), np.zeros(k, np.int32), np.zeros(6, np.int32))
        o, o1 = mk(K), mk(1)
        fk, ff = L.plvs_hip_orb_search_by_bow_kf, L.plvs_hip_orb_search_by_bow_frame_kf
        fk.argtypes = [_vp, _vp, _vp, _vp, _i, _f, _i, _vp, _vp, _vp, _vp, _vp]
        ff.argtypes = [_vp, _vp, _i, _vp, _f, _i, _vp, _vp, _vp, _vp, _vp]
        fkh, ffh = L.plvs_hip_orb_search_by_bow_kf_host, L.plvs_hip_orb_search_by_bow_frame_kf_host
        fkh.argtypes, ffh.argtypes = fk.argtypes[:-1], ff.argtypes[:-1]
        one_h = [(_vp * 1)(h.handle) for h in hb]
        one_v = [(_vp * 1)(v.ctypes.data) for v in vb]
        if kind == "kf":
            one_call = lambda: fk(ha.handle, p(va), hs, vs, K, ratio, 1, *[p(x) for x in o], None)
            host = lambda: fkh(ha.handle, p(va), hs, vs, K, ratio, 1, *[p(x) for x in o])
            single = lambda k: fk(ha.handle, p(va), one_h[k], one_v[k], 1, ratio, 1, *[p(x) for x in o1], None)
        else:
            one_call = lambda: ff(hs, vs, K, ctypes.byref(fc), ratio, 1, *[p(x) for x in o], None)
            host = lambda: ffh(hs, vs, K, ctypes.byref(fc), ratio, 1, *[p(x) for x in o])
            single = lambda k: ff(one_h[k], one_v[k], 1, ctypes.byref(fc), ratio, 1, *[p(x) for x in o1], None)

        def k_single_calls():
            for k in range(K):
                rc = single(k)
                if rc:
                    return rc
            return 0

        # the round-1 entry: (key frame = the serial side, frame = the lane side); the kf kind hands KF2 over as the frame
        old = L.plvs_hip_orb_search_by_bow
        old.argtypes = [_vp, _vp, _i, _vp, _vp, _vp, _vp, _i, _vp, _f, _i, _vp, _vp]
        av, ad, aa = S.feature_vector(a_side), np.ascontiguousarray(a_side["desc"]), np.ascontiguousarray(a_side["angle"])
        ac = av.as_c()
        bvec = [S.feature_vector(b) for b in b_sides]
        bc = [v.as_c() for v in bvec]
        bd, ba = [np.ascontiguousarray(b["desc"]) for b in b_sides], [np.ascontiguousarray(b["angle"]) for b in b_sides]
        nm = _i()

        def k_old_calls():
            for k in range(K):
                nb = len(bd[k])
                assigned = np.zeros(max(n, nb), np.int32)
                if kind == "kf":
                    rc = old(ctypes.byref(ac), p(ad), n, p(va), p(aa), ctypes.byref(bc[k]), p(bd[k]), nb, p(ba[k]), ratio, 1, p(assigned), ctypes.byref(nm))
                else:
                    rc = old(ctypes.byref(bc[k]), p(bd[k]), nb, p(vb[k]), p(ba[k]), ctypes.byref(ac), p(ad), n, p(aa), ratio, 1, p(assigned), ctypes.byref(nm))
                if rc:
                    return rc
            return 0

        calls = dict(one_call=one_call, k_single_calls=k_single_calls, k_calls_of_the_round_1_entry=k_old_calls)
        rounds = {k: [] for k in calls}
        for _ in range(a.rounds):
            for key, call in calls.items():
                rounds[key].append(timed(call, a.calls, a.warmup))
        out["rounds"] = rounds
        out["us_median_of_rounds"] = {k: round(float(np.median([r["us_median"] for r in rounds[k]])), 1) for k in calls}
        out["what"] = dict(one_call="plvs_hip_orb_search_by_bow_kf" if kind == "kf" else "plvs_hip_orb_search_by_bow_frame_kf",
                           k_single_calls=f"{K} calls of the same entry with one key frame each, in a row",
                           k_calls_of_the_round_1_entry=f"{K} calls of plvs_hip_orb_search_by_bow in a row" +
                           (" with KF2 handed over as the frame: its semantics differ (no validity gate on KF2, <= TH_LOW)" if kind == "kf" else ""))
        one_call()
        dev = [x.copy() for x in o[:3]]
        out["result"] = dict(stats=o[3].tolist(), copy_in_bytes=int(o[3][2]), nmatches=o[2].tolist())
        out["host_twin"] = dict(timed(host, 5, 1), what="the _kf_host entry: the same per-job code, serially, on the handles' host copies")
        assert all((x == y).all() for x, y in zip(dev, o[:3])), "the device entry and the host twin disagree"
        if kind == "frame":   # the frame kind and the round-1 entry mean the same: their results are equal
            for k in range(K):
                nb = len(bd[k])
                assigned = np.zeros(n, np.int32)
                _lib.check(old(ctypes.byref(bc[k]), p(bd[k]), nb, p(vb[k]), p(ba[k]), ctypes.byref(ac), p(ad), n, p(aa), ratio, 1, p(assigned), ctypes.byref(nm)))
                assert (assigned == dev[0][k]).all() and nm.value == dev[2][k], "the one-call entry and plvs_hip_orb_search_by_bow disagree"
    finally:
        for h in [ha] + hb:
            h.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="loop_detection,relocalisation")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--calls", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bow_search_timing.json"))
    a = ap.parse_args()
    doc = {}
    if os.path.exists(a.out):
        with open(a.out) as fh:
            doc = json.load(fh)
    doc.update(what="per-call wall clock around the raw C ABI calls (ctypes, structures and handles built once) on one MI355X; every device "
                    "call ends in a stream wait and the host's histogram pass; the entries run alternately in rounds in one process; bench.py "
                    "does not call these entries",
               source="scripts/measure_bow_search.py")
    for name in a.shapes.split(","):
        kind, K, ratio = SHAPES[name]
        doc[name] = shape_figures(kind, K, ratio, a)
        print(name, json.dumps(doc[name]["us_median_of_rounds"]), json.dumps(doc[name]["host_twin"]), json.dumps(doc[name]["result"]["stats"]), flush=True)
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(doc, fh, indent=1)


if __name__ == "__main__":
    main()
