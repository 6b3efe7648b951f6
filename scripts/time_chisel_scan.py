"""Times the projective depth + colour scan integrate (plvs_hip_tsdf_chisel_integrate_scans_dev) on the office loop of
tests/synth_scene.py: full-size 640 x 480 depth / colour images resident in HBM, 5 cm map, HIP events around each call,
5 warm-up + 20 timed steps per setting:
  scan_1       one scan per call (scan k of the loop into the growing map)
  scan_100     scans 0-99 in ONE call into an empty map (the map is cleared outside the timed region)
  scan_100_again   the same 100 scans once more into the map they built (no chunk is created)
and beside them, same device and same run, FOR CONTEXT ONLY (they are other integrators and build other maps): the ray
walk on the same 100 key frames' stride-2 clouds in one call, bit-exact (`ray_ordered_100`) and order-free
(`ray_order_free_100`), each into an empty map.
One JSON document on stdout (and in --out).  --trace: only two scan_100 steps, for
`rocprofv3 --kernel-trace --stats -- python scripts/time_chisel_scan.py --trace`."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from plvs_amd.tsdf import TsdfChisel  # noqa: E402
from tests.synth_scene import TUM1, make_stream_keyframes  # noqa: E402

NEAR, FAR = 0.1, 5.0


def timed(fn, before=None, warmup=5, steps=20):
    ms = []
    for i in range(warmup + steps):
        if before is not None:
            before(i)
            torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn(i)
        b.record()
        torch.cuda.synchronize()
        if i >= warmup:
            ms.append(a.elapsed_time(b))
    ms = np.array(ms)
    return dict(ms_median=round(float(np.median(ms)), 4), ms_p10_p90=[round(float(np.percentile(ms, 10)), 4),
                                                                       round(float(np.percentile(ms, 90)), 4)], steps=len(ms))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--scans", type=int, default=100)
    args = ap.parse_args()
    K = args.scans
    cam = dict(TUM1)
    imgs = make_stream_keyframes(K, step=1, images=True)
    d_depth = torch.from_numpy(np.stack([f["depth_grid"] for f in imgs])).cuda()
    d_bgr = torch.from_numpy(np.stack([f["rgb_grid"] for f in imgs])).cuda()
    d_Twc = torch.from_numpy(np.stack([f["Twc"] for f in imgs])).cuda()
    out = dict(what="scripts/time_chisel_scan.py: HIP-event time per call, 640 x 480 images in HBM, 5 cm, office loop key "
                    f"frames 0-{K - 1}", device=torch.cuda.get_device_name(0), scans_per_call=K)
    m = TsdfChisel(0.05, max_chunks=8192)

    def scan_all(_):
        m.integrate_scans_dev(d_depth, d_bgr, cam, d_Twc, near=NEAR, far=FAR)

    if args.trace:
        for _ in range(2):
            m.clear()
            scan_all(0)
        out["scan_100_stats"] = m.last_stats()
        out["chunks"] = m.num_chunks()
        print(json.dumps(out))
        return
    out["scan_100"] = timed(scan_all, before=lambda i: m.clear())
    out["scan_100"].update(stats=m.last_stats(), chunks=m.num_chunks())
    out["scan_100_again"] = timed(scan_all)
    out["scan_100_again"].update(stats=m.last_stats(), chunks=m.num_chunks())
    m.clear()
    out["scan_1"] = timed(lambda i: m.integrate_scans_dev(d_depth[i:i + 1], d_bgr[i:i + 1], cam, d_Twc[i:i + 1], near=NEAR, far=FAR))
    out["scan_1"].update(stats=m.last_stats(), chunks=m.num_chunks())
    m.close()
    del d_depth, d_bgr

    # ---- context: the ray walk on the same key frames (stride-2 clouds, as PointCloudMapping makes them)
    kfs = make_stream_keyframes(K, step=2)
    offsets = np.concatenate([[0], np.cumsum([len(k["xyz"]) for k in kfs])]).astype(np.int32)
    d_xyz = torch.from_numpy(np.concatenate([k["xyz"] for k in kfs])).cuda()
    d_rgb = torch.from_numpy(np.concatenate([k["rgb"] for k in kfs])).cuda()
    d_kfid = torch.from_numpy(np.concatenate([k["kfid"] for k in kfs]).astype(np.int32)).cuda()
    d_T = torch.from_numpy(np.stack([k["Twc"] for k in kfs])).cuda()
    for name, order_free in (("ray_ordered_100", False), ("ray_order_free_100", True)):
        r = TsdfChisel(0.05, max_chunks=8192, order_free=order_free)
        out[name] = timed(lambda i: r.integrate_batch_dev(d_xyz, d_rgb, d_kfid, offsets, d_T), before=lambda i: r.clear())
        out[name].update(stats=r.last_stats(), chunks=r.num_chunks(), points=int(offsets[-1]))
        r.close()
    print(json.dumps(out))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
