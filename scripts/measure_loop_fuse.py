#!/usr/bin/env python3
"""Per-call time of the Sim3 Fuse searches of LoopClosing::SearchAndFuse over resident key frames -> profiles/loop_fuse_timing.json.

Shapes (chosen ones: the reference's sizes depend on the data):
  nominal   30 handles x 10 000 loop points x 1500 key points and 30 x 2 000 loop lines x 300 key lines, the key frames on a ring
            (tests/loop_fuse_scenario.nominal_point_inputs / nominal_line_inputs): a minority of the pairs survives the projection's
            tests; the fraction the generator gives is recorded (survivor_fraction, from the reached codes of the call itself);
  small     5 x 1500 x 1500 of the same generator.
Figures, th 4: the point search in the sieve layout and in the wave-per-pair layout (plvs_hip_loop_fuse_test_layout 0 / 1), the two run
alternately --rounds times in one process; the line search; both kinds in one call; 30 single-key-frame point calls in a row (what
a caller without the batch pays); the two host entries.  The clock is the host's around the raw ABI calls, which end in a stream
wait; the C structures and the handles are made before it starts.  Median of --calls after --warmup with p10 and p90 per round: the
spread between rounds of one layout stands beside the difference between the layouts.  scripts/make_loop_fuse_golden.py --time adds
"cpu_reference" to the same file.  No threshold is asserted anywhere; bench.py does not call these entries."""
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
SHAPES = dict(nominal=((30, 10000, 1500), (30, 2000, 300)), small=((5, 1500, 1500), None))


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


def shape_figures(name, a):
    from plvs_amd import _lib
    from plvs_amd.keyframe import _lists, loop_fuse_test_layout
    from tests import loop_fuse_scenario as S
    import torch
    assert torch.cuda.is_available(), "a measurement needs the GPU"
    L, p = _lib.lib, _lib.np_ptr
    pshape, lshape = SHAPES[name]
    pin = S.nominal_point_inputs(*pshape)
    lin = S.nominal_line_inputs(*lshape) if lshape else None
    K = pshape[0]
    out = dict(shape=dict(points="%d handles x %d loop points x %d key points" % pshape,
                          lines=None if lshape is None else "%d handles x %d loop lines x %d key lines" % lshape), th=S.TH,
               device=torch.cuda.get_device_name(0))
    single = [_vp, _vp, _i, _vp, _vp, _f, _vp, _vp, _vp, _vp]
    mk = lambda m: (np.zeros((K, m), np.int32), np.zeros((K, m), np.int32), np.zeros((K, m), np.uint8), np.zeros(4, np.int32))
    ptrs = lambda o: [p(x) for x in o]
    with S.Handles(points_inp=pin, lines_inp=lin) as h:
        _, hs, ps = _lists(h.kfs, S.poses(pin["kfs"]))         # the point search at the point set's own poses
        pc = h.points.as_c()
        psk = np.ascontiguousarray(pin["skip"], np.uint8)
        po = mk(pc.m)
        f = L.plvs_hip_orb_loop_fuse_search_kf
        f.argtypes = single + [_vp]
        point_call = lambda: f(hs, ps, K, ctypes.byref(pc), p(psk), S.TH, *ptrs(po), None)
        rounds = {"sieve": [], "wave_per_pair": []}
        results = {}
        for _ in range(a.rounds):
            for layout, key in ((0, "sieve"), (1, "wave_per_pair")):
                loop_fuse_test_layout(layout)
                rounds[key].append(timed(point_call, a.calls, a.warmup))
                results[key] = [x.copy() for x in po[:3]]
        loop_fuse_test_layout(0)
        assert all((x == y).all() for x, y in zip(results["sieve"], results["wave_per_pair"])), "the two layouts disagree"
        reached = po[2]
        unskipped = int((reached != 0).sum())
        out["points"] = dict(rounds=rounds, stats=po[3].tolist(), candidates=int((reached == 9).sum()), pairs=int(reached.size),
                             survivor_fraction=round(float((reached >= 6).sum()) / max(unskipped, 1), 4),
                             what="plvs_hip_orb_loop_fuse_search_kf, the two layouts alternately; survivor_fraction: pairs that passed the "
                                  "projection's tests over the pairs not skipped")
        med = lambda key: float(np.median([r["us_median"] for r in rounds[key]]))
        out["points"]["sieve_over_wave_per_pair"] = round(med("sieve") / med("wave_per_pair"), 3)
        # one key frame per call, 30 calls in a row
        one = (np.zeros((1, pc.m), np.int32), np.zeros((1, pc.m), np.int32), np.zeros((1, pc.m), np.uint8), np.zeros(4, np.int32))
        rows = [np.ascontiguousarray(psk[k:k + 1]) for k in range(K)]
        hk = [(_vp * 1)(h.kfs[k].handle) for k in range(K)]
        pk = [_lists([h.kfs[k]], [S.poses(pin["kfs"])[k]])[2] for k in range(K)]

        def single_calls():
            for k in range(K):
                rc = f(hk[k], pk[k], 1, ctypes.byref(pc), p(rows[k]), S.TH, *ptrs(one), None)
                if rc:
                    return rc
            return 0
        out["points_single_key_frame_calls"] = dict(timed(single_calls, max(a.calls // 4, 5), 3), what=f"{K} calls of one key frame each, in a row")
        fh = L.plvs_hip_orb_loop_fuse_search_kf_host
        fh.argtypes = single
        out["points_host"] = dict(timed(lambda: fh(hs, ps, K, ctypes.byref(pc), p(psk), S.TH, *ptrs(po)), 3, 1),
                                  what="plvs_hip_orb_loop_fuse_search_kf_host, serial, on the handles' host copies")
        if lin is not None:
            _, _, ls = _lists(h.kfs, S.poses(lin["kfs"]))
            lc = h.lines.as_c()
            lsk = np.ascontiguousarray(lin["skip"], np.uint8)
            lo = mk(lc.m)
            g = L.plvs_hip_line_loop_fuse_search_kf
            g.argtypes = single + [_vp]
            out["lines"] = dict(timed(lambda: g(hs, ls, K, ctypes.byref(lc), p(lsk), S.TH, *ptrs(lo), None), a.calls, a.warmup),
                                stats=lo[3].tolist(), candidates=int((lo[2] == 12).sum()), pairs=int(lo[2].size),
                                survivor_fraction=round(float((lo[2] >= 9).sum()) / max(int((lo[2] != 0).sum()), 1), 4))
            gh = L.plvs_hip_line_loop_fuse_search_kf_host
            gh.argtypes = single
            out["lines_host"] = timed(lambda: gh(hs, ls, K, ctypes.byref(lc), p(lsk), S.TH, *ptrs(lo)), 3, 1)
            both = L.plvs_hip_loop_fuse_search_points_and_lines_kf
            both.argtypes = [_vp, _vp, _i, _vp, _vp, _f, _vp, _vp, _vp, _vp, _vp, _vp, _f, _vp, _vp, _vp, _vp, _vp, _vp]
            st = np.zeros(3, np.int32)
            out["both"] = dict(timed(lambda: both(hs, ls, K, ctypes.byref(pc), p(psk), S.TH, *ptrs(po), ctypes.byref(lc), p(lsk), S.TH, *ptrs(lo),
                                                  p(st), None), a.calls, a.warmup), call_stats=st.tolist(),
                               what="both kinds in one call at the line set's poses (the points then see another pose than in `points`)")
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="nominal,small")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--calls", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "loop_fuse_timing.json"))
    a = ap.parse_args()
    doc = {}
    if os.path.exists(a.out):
        with open(a.out) as fh:
            doc = json.load(fh)
    doc.update(what="per-call wall clock around the raw C ABI calls (ctypes, structures and handles built once) on one MI355X; every device "
                    "call ends in a stream wait; the two point layouts run alternately in one process; bench.py does not call these entries",
               source="scripts/measure_loop_fuse.py")
    for name in a.shapes.split(","):
        doc[name] = shape_figures(name, a)
        print(name, json.dumps(doc[name]), flush=True)
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(doc, fh, indent=1)


if __name__ == "__main__":
    main()
