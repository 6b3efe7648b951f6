#!/usr/bin/env python3
"""Per-call time of the line Fuse search -> profiles/line_fuse_timing.json (beside the "cpu_reference" figure
scripts/make_line_fuse_golden.py --time measured on one core), at 30 key frames x 300 map lines x 300 key lines
(tests/line_fuse_scenario.random_inputs(30, 300, 300, seed=9)), th 3:
  --mode batched    plvs_hip_line_fuse_search, every key frame in one call
  --mode per_kf     30 calls with n_kfs == 1
  --mode host       plvs_hip_line_fuse_search_host on one core (no device)
  --mode combined   plvs_hip_fuse_search_points_and_lines: the points of 30 x 1500 x 1500 (tests/orb_fuse_scenario.random_inputs,
                    the shape of profiles/orb_fuse_timing.json) and these lines in one call, one wait
  --mode back_to_back   plvs_hip_orb_fuse_search, then plvs_hip_line_fuse_search, on the same two workloads: two waits
Each mode is meant to run in a fresh process.  The C structures are built once; the clock is the host's around the raw ABI calls,
which end in a stream wait.  Median of --calls after --warmup, with p10 and p90.  Beside the times: how many pairs reach a window,
the mean window population (the restatement's count, one key frame's worth) and the pairs the host decided."""
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


def window_population(inp):
    """Mean number of key lines GetLineFeaturesInArea returns, over the windows of key frame 0 (the restatement's walk)."""
    from tests import line_fuse_restatement as R
    kf = inp["kfs"][0]
    grid, fr = R.grid_of(kf), R.front(kf, inp["lines"])
    sizes = []
    for i in np.flatnonzero(fr["reached"] == R.EMPTY_WINDOW):
        nx, ny, d, n2 = R.representation(fr["uS"][i], fr["vS"][i], fr["uE"][i], fr["vE"][i])
        if n2 == 0:
            continue
        level = R.predict_scale(fr["ratio"][i], np.float32(kf["log_scale_factor"]), len(kf["scale_factors"]))[0]
        sc = np.asarray(kf["scale_factors"], np.float32)[level]
        ind, _ = R.window(kf, grid, R.atan2_host(ny, nx), d, np.float32(R.K_DELTA_THETA * sc), np.float32(np.float32(np.float32(inp["th"]) * R.K_DELTA_D) * sc))
        sizes.append(len(ind))
    return round(float(np.mean(sizes)), 1) if sizes else 0.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=("batched", "per_kf", "host", "combined", "back_to_back"), required=True)
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--shape", default="30,300,300")
    ap.add_argument("--point-shape", default="30,1500,1500")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "line_fuse_timing.json"))
    a = ap.parse_args()
    from tests import line_fuse_scenario as S
    K, M, N = (int(c) for c in a.shape.split(","))
    inp = S.random_inputs(K, M, N, seed=9)
    from plvs_amd import _lib
    from plvs_amd import linematcher as LM
    L, p = _lib.lib, _lib.np_ptr
    kfs, lines = S.views(inp)
    ck = [kf.as_c() for kf in kfs]
    arr = (LM._LineFuseKeyFrameC * K)(*ck)
    singles = [(LM._LineFuseKeyFrameC * 1)(c) for c in ck]
    lc = lines.as_c()
    skip = np.ascontiguousarray(inp["skip"], np.uint8)
    bi, bd, rc, st = np.zeros((K, M), np.int32), np.zeros((K, M), np.int32), np.zeros((K, M), np.uint8), np.zeros(3, np.int32)
    dev = L.plvs_hip_line_fuse_search
    dev.argtypes = [_vp, _i, _vp, _vp, _f, _vp, _vp, _vp, _vp, _vp]
    host = L.plvs_hip_line_fuse_search_host
    host.argtypes = [_vp, _i, _vp, _vp, _f, _vp, _vp, _vp, _vp]
    with_points = a.mode in ("combined", "back_to_back")
    if with_points:
        from plvs_amd import orbmatcher as O
        from tests import orb_fuse_scenario as PS
        PK, PM, PN = (int(c) for c in a.point_shape.split(","))
        pin = PS.random_inputs(PK, PM, PN, seed=9)
        pkfs, pts = PS.views(pin)
        parr = (O._FuseKeyFrameC * PK)(*[kf.as_c() for kf in pkfs])
        pc = pts.as_c()
        pskip = np.ascontiguousarray(pin["skip"], np.uint8)
        pbi, pbd, prc, pst = np.zeros((PK, PM), np.int32), np.zeros((PK, PM), np.int32), np.zeros((PK, PM), np.uint8), np.zeros(3, np.int32)
        pdev = L.plvs_hip_orb_fuse_search
        pdev.argtypes = [_vp, _i, _vp, _vp, _f, _vp, _vp, _vp, _vp, _vp]
        both = L.plvs_hip_fuse_search_points_and_lines
        both.argtypes = [_vp, _i, _vp, _vp, _f, _vp, _vp, _vp, _vp, _vp, _i, _vp, _vp, _f, _vp, _vp, _vp, _vp, _vp, _vp]
        bst = np.zeros(2, np.int32)

    def batched():
        _lib.check(dev(arr, K, ctypes.byref(lc), p(skip), 3.0, p(bi), p(bd), p(rc), p(st), None))

    def per_kf():
        for k in range(K):
            _lib.check(dev(singles[k], 1, ctypes.byref(lc), p(skip[k]), 3.0, p(bi[k]), p(bd[k]), p(rc[k]), p(st), None))

    def on_host():
        _lib.check(host(arr, K, ctypes.byref(lc), p(skip), 3.0, p(bi), p(bd), p(rc), p(st)))

    def combined():
        _lib.check(both(parr, PK, ctypes.byref(pc), p(pskip), 3.0, p(pbi), p(pbd), p(prc), p(pst), arr, K, ctypes.byref(lc), p(skip), 3.0, p(bi),
                        p(bd), p(rc), p(st), p(bst), None))

    def back_to_back():
        _lib.check(pdev(parr, PK, ctypes.byref(pc), p(pskip), 3.0, p(pbi), p(pbd), p(prc), p(pst), None))
        batched()

    fn = dict(batched=batched, per_kf=per_kf, host=on_host, combined=combined, back_to_back=back_to_back)[a.mode]
    device = None
    if a.mode != "host":
        import torch
        assert torch.cuda.is_available(), "a measurement needs the GPU"
        device = torch.cuda.get_device_name(0)
    us = []
    for k in range(a.warmup + a.calls):
        t0 = time.perf_counter()
        fn()
        us.append((time.perf_counter() - t0) * 1e6)
    workload = f"{K} key frames x {M} map lines x {N} key lines (tests/line_fuse_scenario.random_inputs, seed 9), th 3"
    if with_points:
        workload += f"; points: {PK} key frames x {PM} points x {PN} key points (tests/orb_fuse_scenario.random_inputs, seed 9), th 3"
    result = dict(stats(us[a.warmup:]), workload=workload, stats=[int(s) for s in st])
    if a.mode == "per_kf":
        result["stats_note"] = "stats of the last of the 30 calls"
    if with_points:
        result["point_stats"] = [int(s) for s in pst]
        if a.mode == "combined":
            result["call_stats"] = [int(s) for s in bst]
    measured = (bi.copy(), bd.copy(), rc.copy())
    on_host()
    assert all((x == y).all() for x, y in zip(measured, (bi, bd, rc))), "the measured mode and the host entry disagree"
    result["candidates"] = int((rc == 12).sum())
    result["pairs"] = int(rc.size)
    result["pairs_reaching_a_window"] = int((rc >= 9).sum())
    if a.mode in ("batched", "host"):
        result["mean_window_population_kf0"] = window_population(inp)
    doc = {}
    if os.path.exists(a.out):
        with open(a.out) as fh:
            doc = json.load(fh)
    if device is None:
        doc["host_entry"] = dict(result, what="plvs_hip_line_fuse_search_host, one core, on the machine that ran the GPU figures", source="scripts/measure_line_fuse.py")
    else:
        gpu = doc.setdefault("gpu", dict(what="per-call wall clock around the raw C ABI calls (ctypes, structures built once) on one MI355X; every "
                                              "call ends in a stream wait; a fresh process per figure", source="scripts/measure_line_fuse.py"))
        gpu["device"] = device
        gpu[a.mode] = result
    with open(a.out, "w") as fh:
        json.dump(doc, fh, indent=1)
    print(a.mode, json.dumps(result))


if __name__ == "__main__":
    main()
