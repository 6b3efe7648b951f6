#!/usr/bin/env python3
"""Per-call time of the Fuse search -> profiles/orb_fuse_timing.json (beside the "cpu_reference" figure scripts/make_orb_fuse_golden.py
--time measured on one core), at 30 key frames x 1500 points x 1500 key points (tests/orb_fuse_scenario.random_inputs(30, 1500, 1500,
seed=9)), th 3:
  --mode batched          plvs_hip_orb_fuse_search, every key frame in one call, the projection inside the window launch
  --mode batched_chained  the same with the projection as a thread-per-pair launch chained in front (plvs_hip_orb_fuse_test_chained(1))
  --mode copy_in          the staging and the copy in alone (plvs_hip_orb_fuse_test_chained(2)): what key frames resident in HBM
                           would remove
  --mode per_kf           30 calls with n_kfs == 1
  --mode host             plvs_hip_orb_fuse_search_host on one core (no device)
Each mode is meant to run in a fresh process.  The C structures are built once; the clock is the host's around the raw ABI calls,
which end in a stream wait.  Median of --calls after --warmup, with p10 and p90."""
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
    ap.add_argument("--mode", choices=("batched", "batched_chained", "copy_in", "per_kf", "host"), required=True)
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--shape", default="30,1500,1500")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "orb_fuse_timing.json"))
    a = ap.parse_args()
    from tests import orb_fuse_scenario as S
    K, M, N = (int(c) for c in a.shape.split(","))
    inp = S.random_inputs(K, M, N, seed=9)
    from plvs_amd import _lib
    from plvs_amd import orbmatcher as O
    L, p = _lib.lib, _lib.np_ptr
    kfs, pts = S.views(inp)
    ck = [kf.as_c() for kf in kfs]
    arr = (O._FuseKeyFrameC * K)(*ck)
    singles = [(O._FuseKeyFrameC * 1)(c) for c in ck]
    pc = pts.as_c()
    skip = np.ascontiguousarray(inp["skip"], np.uint8)
    bi, bd, rc, st = np.zeros((K, M), np.int32), np.zeros((K, M), np.int32), np.zeros((K, M), np.uint8), np.zeros(3, np.int32)
    dev = L.plvs_hip_orb_fuse_search
    dev.argtypes = [_vp, _i, _vp, _vp, _f, _vp, _vp, _vp, _vp, _vp]
    host = L.plvs_hip_orb_fuse_search_host
    host.argtypes = [_vp, _i, _vp, _vp, _f, _vp, _vp, _vp, _vp]

    def batched():
        _lib.check(dev(arr, K, ctypes.byref(pc), p(skip), 3.0, p(bi), p(bd), p(rc), p(st), None))

    def per_kf():
        for k in range(K):
            _lib.check(dev(singles[k], 1, ctypes.byref(pc), p(skip[k]), 3.0, p(bi[k]), p(bd[k]), p(rc[k]), p(st), None))

    def on_host():
        _lib.check(host(arr, K, ctypes.byref(pc), p(skip), 3.0, p(bi), p(bd), p(rc), p(st)))

    fn = dict(batched=batched, batched_chained=batched, copy_in=batched, per_kf=per_kf, host=on_host)[a.mode]
    device = None
    if a.mode != "host":
        import torch
        assert torch.cuda.is_available(), "a measurement needs the GPU"
        device = torch.cuda.get_device_name(0)
    O.fuse_test_chained(dict(batched_chained=1, copy_in=2).get(a.mode, 0))
    us = []
    for k in range(a.warmup + a.calls):
        t0 = time.perf_counter()
        fn()
        us.append((time.perf_counter() - t0) * 1e6)
    O.fuse_test_chained(0)
    result = dict(stats(us[a.warmup:]), workload=f"{K} key frames x {M} points x {N} key points (tests/orb_fuse_scenario.random_inputs, seed 9), th 3",
                  stats=[int(s) for s in st])
    if a.mode != "copy_in":
        on_host_ref = (bi.copy(), bd.copy(), rc.copy())
        on_host()
        assert all((x == y).all() for x, y in zip(on_host_ref, (bi, bd, rc))), "the measured mode and the host entry disagree"
        result["candidates"] = int((rc == 9).sum())
    doc = {}
    if os.path.exists(a.out):
        with open(a.out) as fh:
            doc = json.load(fh)
    if device is None:
        doc["host_entry"] = dict(result, what="plvs_hip_orb_fuse_search_host, one core, on the machine that ran the GPU figures", source="scripts/measure_orb_fuse.py")
    else:
        gpu = doc.setdefault("gpu", dict(what="per-call wall clock around the raw C ABI calls (ctypes, structures built once) on one MI355X; every "
                                              "call ends in a stream wait; a fresh process per figure", source="scripts/measure_orb_fuse.py"))
        gpu["device"] = device
        gpu[a.mode] = result
    with open(a.out, "w") as fh:
        json.dump(doc, fh, indent=1)
    print(a.mode, json.dumps(result))


if __name__ == "__main__":
    main()
