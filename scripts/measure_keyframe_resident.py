#!/usr/bin/env python3
"""Per-call time of the Fuse searches over resident key frames beside the non-resident entries -> profiles/keyframe_resident_timing.json,
at the shapes of DESIGN 6.5 and 6.6: 30 key frames x 1500 points x 1500 key points (tests/orb_fuse_scenario.random_inputs(30, 1500,
1500, seed=9)), 30 x 300 lines x 300 key lines (tests/line_fuse_scenario.random_inputs(30, 300, 300, seed=9)), th 3, and both together.

  measure_keyframe_resident.py [--parent-lib PATH] [--rounds 2]      the sitting: every figure below, a fresh process per figure, each
                                                                    under its own timeout, the three flavours of a kind run alternately;
                                                                    it ends at the first figure that fails
  measure_keyframe_resident.py --figure KIND:FLAVOUR                 one figure (what the sitting starts)
      KIND     points | lines | both
      FLAVOUR  kf          the _kf entry over handles created before the clock starts
               staged      the non-resident entry of the same build
               parent      the non-resident entry of the library PLVS_HIP_LIB names (the parent commit's build, same machine, same
                           sitting: the walk body both kernels now share did not move it)
               create      plvs_hip_keyframe_create + destroy per key frame (points: the point side alone; both: points + lines),
                           with the handle's device and host bytes
The clock is the host's around the raw ABI calls, which end in a stream wait; the C structures are built once.  Median of --calls after
--warmup, with p10 and p90.  bench.py does not call these entries."""
import argparse
import ctypes
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
_vp, _i, _f = ctypes.c_void_p, ctypes.c_int, ctypes.c_float
FIGURES = [(k, f) for k in ("points", "lines", "both") for f in ("kf", "staged", "parent")] + [("points", "create"), ("both", "create")]
POINT_SHAPE, LINE_SHAPE = (30, 1500, 1500), (30, 300, 300)


def stats(us):
    us = np.asarray(us)
    return dict(us_median=round(float(np.median(us)), 1), us_p10=round(float(np.percentile(us, 10)), 1),
                us_p90=round(float(np.percentile(us, 90)), 1), calls=int(len(us)))


def figure(kind, flavour, calls, warmup):
    from plvs_amd import _lib
    from plvs_amd import linematcher as LM
    from plvs_amd import orbmatcher as OM
    from tests import line_fuse_scenario as LS
    from tests import orb_fuse_scenario as PS
    import torch
    assert torch.cuda.is_available(), "a measurement needs the GPU"
    L, p = _lib.lib, _lib.np_ptr
    K = POINT_SHAPE[0]
    pin, lin = PS.random_inputs(*POINT_SHAPE, seed=9), LS.random_inputs(*LINE_SHAPE, seed=9)
    pk, pts = PS.views(pin)
    lk, lines = LS.views(lin)
    pc, lc = pts.as_c(), lines.as_c()
    psk, lsk = np.ascontiguousarray(pin["skip"], np.uint8), np.ascontiguousarray(lin["skip"], np.uint8)
    mk = lambda m, n: (np.zeros((K, m), np.int32), np.zeros((K, m), np.int32), np.zeros((K, m), np.uint8), np.zeros(n, np.int32))
    po, lo, st = mk(pc.m, 4), mk(lc.m, 4), np.zeros(3, np.int32)
    out = lambda o: [p(a) for a in o]
    result = dict(workload=dict(points="%d key frames x %d points x %d key points" % POINT_SHAPE, lines="%d key frames x %d lines x %d key lines" % LINE_SHAPE,
                                both="the two together, one key-frame list")[kind] + ", th 3")
    handles = []
    if flavour in ("kf", "create"):
        from plvs_amd.keyframe import KeyFramePose, ResidentKeyFrame, _lists
        sides = lambda k: dict(points=pk[k] if kind != "lines" else None, lines=lk[k] if kind != "points" else None)
        if flavour == "create":
            us = []
            for k in list(range(K)) * 3:
                t0 = time.perf_counter()
                h = ResidentKeyFrame(**sides(k))
                us.append((time.perf_counter() - t0) * 1e6)
                info = h.info()
                h.close()
            result.update(stats(us[K:]), what="ResidentKeyFrame(...) per key frame, the ctypes structures included; the first pass over the key frames is the warm-up",
                          device_bytes=info["device_bytes"], host_bytes=info["host_bytes"])
            return result
        handles = [ResidentKeyFrame(**sides(k)) for k in range(K)]
        # one pose per key frame for both kinds: each kind is measured at its own scenario's pose (the combined call's points at the lines')
        poses = [KeyFramePose(pk[k].q_cw, lk[k].Rcw, lk[k].tcw if kind != "points" else pk[k].tcw, lk[k].Ow if kind != "points" else pk[k].Ow) for k in range(K)]
        _, hs, ps = _lists(handles, poses)
        info = handles[0].info()
        result.update(device_bytes_per_handle=info["device_bytes"], host_bytes_per_handle=info["host_bytes"])
        if kind == "points":
            f = L.plvs_hip_orb_fuse_search_kf
            f.argtypes = [_vp, _vp, _i, _vp, _vp, _f, _vp, _vp, _vp, _vp, _vp]
            call = lambda: f(hs, ps, K, ctypes.byref(pc), p(psk), 3.0, *out(po), None)
        elif kind == "lines":
            f = L.plvs_hip_line_fuse_search_kf
            f.argtypes = [_vp, _vp, _i, _vp, _vp, _f, _vp, _vp, _vp, _vp, _vp]
            call = lambda: f(hs, ps, K, ctypes.byref(lc), p(lsk), 3.0, *out(lo), None)
        else:
            f = L.plvs_hip_fuse_search_points_and_lines_kf
            f.argtypes = [_vp, _vp, _i, _vp, _vp, _f, _vp, _vp, _vp, _vp, _vp, _vp, _f, _vp, _vp, _vp, _vp, _vp, _vp]
            call = lambda: f(hs, ps, K, ctypes.byref(pc), p(psk), 3.0, *out(po), ctypes.byref(lc), p(lsk), 3.0, *out(lo), p(st), None)
    else:
        parr = (OM._FuseKeyFrameC * K)(*[kf.as_c() for kf in pk])
        larr = (LM._LineFuseKeyFrameC * K)(*[kf.as_c() for kf in lk])
        if kind == "points":
            f = L.plvs_hip_orb_fuse_search
            f.argtypes = [_vp, _i, _vp, _vp, _f, _vp, _vp, _vp, _vp, _vp]
            call = lambda: f(parr, K, ctypes.byref(pc), p(psk), 3.0, *out(po), None)
        elif kind == "lines":
            f = L.plvs_hip_line_fuse_search
            f.argtypes = [_vp, _i, _vp, _vp, _f, _vp, _vp, _vp, _vp, _vp]
            call = lambda: f(larr, K, ctypes.byref(lc), p(lsk), 3.0, *out(lo), None)
        else:
            f = L.plvs_hip_fuse_search_points_and_lines
            f.argtypes = [_vp, _i, _vp, _vp, _f, _vp, _vp, _vp, _vp, _vp, _i, _vp, _vp, _f, _vp, _vp, _vp, _vp, _vp, _vp]
            call = lambda: f(parr, K, ctypes.byref(pc), p(psk), 3.0, *out(po), larr, K, ctypes.byref(lc), p(lsk), 3.0, *out(lo), p(st), None)
    us = []
    for _ in range(warmup + calls):
        t0 = time.perf_counter()
        rc = call()
        us.append((time.perf_counter() - t0) * 1e6)
        _lib.check(rc)
    result.update(stats(us[warmup:]), library="the parent commit's build (PLVS_HIP_LIB)" if flavour == "parent" else "this build")
    if kind != "lines":
        result.update(point_stats=po[3].tolist(), point_candidates=int((po[2] == 9).sum()))
    if kind != "points":
        result.update(line_stats=lo[3].tolist(), line_candidates=int((lo[2] == 12).sum()))
    if kind == "both":
        result["call_stats"] = st.tolist()
    if flavour == "kf":
        result["copy_in_bytes"] = int(st[2]) if kind == "both" else int((po if kind == "points" else lo)[3][3])
    for h in handles:
        h.close()
    result["device"] = torch.cuda.get_device_name(0)
    return result


def sitting(a):
    doc = dict(what="per-call wall clock around the raw C ABI calls (ctypes, structures built once) on one MI355X; every call ends in a stream wait; "
                    "a fresh process per figure, the flavours of a kind run alternately, --rounds times; bench.py does not call these entries",
               source="scripts/measure_keyframe_resident.py", figures={})
    for rnd in range(a.rounds):
        for kind, flavour in FIGURES:
            if flavour == "parent" and not a.parent_lib:
                continue
            if flavour == "create" and rnd:
                continue
            env = dict(os.environ)
            if flavour == "parent":
                env["PLVS_HIP_LIB"] = os.path.abspath(a.parent_lib)
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--figure", f"{kind}:{flavour}", "--calls", str(a.calls), "--warmup", str(a.warmup)],
                               env=env, capture_output=True, text=True, timeout=a.step_timeout)
            if r.returncode != 0:      # nothing more is started on the device after a figure that failed
                sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
                raise SystemExit(f"{kind}:{flavour} ended with {r.returncode}")
            res = json.loads(r.stdout.strip().splitlines()[-1])
            doc["figures"].setdefault(f"{kind}_{flavour}", []).append(res)
            print(kind, flavour, json.dumps(res), flush=True)
            with open(a.out, "w") as fh:
                json.dump(doc, fh, indent=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--figure")
    ap.add_argument("--parent-lib")
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--step-timeout", type=int, default=120)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "keyframe_resident_timing.json"))
    a = ap.parse_args()
    if a.figure:
        kind, flavour = a.figure.split(":")
        print(json.dumps(figure(kind, flavour, a.calls, a.warmup)))
    else:
        sitting(a)


if __name__ == "__main__":
    main()
