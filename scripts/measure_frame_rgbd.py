#!/usr/bin/env python3
"""Per-call times of the RGB-D frame entries on the GPU -> profiles/frame_rgbd_timing.json (beside the "cpu_reference" figure
scripts/make_frame_rgbd_golden.py measured):
  dev_flavour   plvs_hip_frame_stereo_from_rgbd_dev, 2000 key points + 100 lines on 640 x 480, depth resident in HBM
  host_flavours the two host flavours on the same inputs (each uploads the image)
  one_call      plvs_hip_frame_rgbd_dev against the sum of its pieces called one by one, 640 x 480 golden image
Host clock around calls that end in a stream wait (the outputs are host arrays); warm-up first; the two variants of a
comparison alternate inside one loop.  Usage: measure_frame_rgbd.py [--calls 300] [--out profiles/frame_rgbd_timing.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def stats(us):
    us = np.asarray(us)
    return dict(us_median=round(float(np.median(us)), 1), us_p10=round(float(np.percentile(us, 10)), 1),
                us_p90=round(float(np.percentile(us, 90)), 1), calls=int(len(us)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=300)
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "frame_rgbd_timing.json"))
    a = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "a measurement needs the GPU"
    from plvs_amd import frame
    from plvs_amd.lines import LineExtractor
    from plvs_amd.orb import ORBextractor
    from tests import frame_rgbd_scenario as S
    from tests.oracle_lib import golden
    from tests.test_frame_rgbd import MBF, TUM1_D, TUM1_K, _synthetic_depth

    def clock(fn):
        t0 = time.perf_counter()
        fn()
        return (time.perf_counter() - t0) * 1e6

    inp = S.timing_inputs()
    d_depth = torch.from_numpy(inp["depth"]).cuda()
    torch.cuda.synchronize()
    args = (inp["K4"], inp["mbf"], inp["min_line_length_3d"])
    dev = lambda: frame.stereo_from_rgbd(inp["kps"], inp["kps_un"], inp["keylines"], inp["keylines_un"], d_depth, *args)    # noqa: E731
    host = lambda: (frame.ComputeStereoFromRGBD(inp["kps"], inp["kps_un"], inp["depth"], inp["mbf"]),                        # noqa: E731
                    frame.ComputeStereoLinesFromRGBD(inp["keylines"], inp["keylines_un"], inp["depth"], *args))
    # the two must agree before either is timed
    for x, y in zip(dev(), host()[0] + host()[1]):
        assert np.array_equal(x.view(np.uint32), y.view(np.uint32))
    t_dev, t_host = [], []
    for k in range(a.warmup + a.calls):
        td, th = clock(dev), clock(host)
        if k >= a.warmup:
            t_dev.append(td)
            t_host.append(th)

    grey = golden("aloe_640x480.pgm")
    h, w = grey.shape
    image = torch.from_numpy(grey).cuda()
    depth = torch.from_numpy(_synthetic_depth(h, w, w)).cuda()
    b = frame.ComputeImageBounds(w, h, TUM1_K, TUM1_D)
    gw, gh = np.float32(64) / (np.float32(b[1]) - np.float32(b[0])), np.float32(48) / (np.float32(b[3]) - np.float32(b[2]))
    orb, lines = ORBextractor(1000, 1.2, 8, 20, 7), LineExtractor(100)
    one = lambda: frame.rgbd_frame(orb, lines, image, depth, TUM1_K, TUM1_D, MBF, b[:4], gw, gh)                             # noqa: E731
    piece_names = ("extract_frame", "UndistortKeyPoints", "ComputeStereoFromRGBD", "UndistortKeyLines", "ComputeStereoLinesFromRGBD",
                   "AssignFeaturesToGrid")
    t_one, t_pieces = [], {k: [] for k in piece_names}
    counts = None
    for k in range(a.warmup + a.calls):
        to = clock(one)
        s = {}
        t0 = time.perf_counter()
        mono, kps, desc, kl, kld = frame.extract_frame(orb, lines, image)
        t1 = time.perf_counter()
        un = frame.UndistortKeyPoints(kps, TUM1_K, TUM1_D)
        t2 = time.perf_counter()
        frame.ComputeStereoFromRGBD(kps, un, depth, MBF)
        t3 = time.perf_counter()
        klu, kept = frame.UndistortKeyLines(kl, TUM1_K, TUM1_D, b[:4])
        kl, kld = kl[kept], kld[kept]
        t4 = time.perf_counter()
        frame.ComputeStereoLinesFromRGBD(kl, klu, depth, TUM1_K, MBF)
        t5 = time.perf_counter()
        frame.AssignFeaturesToGrid(un, b[0], b[2], gw, gh)
        t6 = time.perf_counter()
        counts = dict(key_points=len(kps), lines=len(kl))
        if k >= a.warmup:
            t_one.append(to)
            for name, (x, y) in zip(piece_names, ((t0, t1), (t1, t2), (t2, t3), (t3, t4), (t4, t5), (t5, t6))):
                t_pieces[name].append((y - x) * 1e6)
    total = np.sum([t_pieces[k] for k in piece_names], 0)
    doc = {}
    src = os.path.join(ROOT, "profiles", "frame_rgbd_timing.json")
    if os.path.exists(src):
        with open(src) as fh:
            doc = json.load(fh)
    doc["gpu"] = dict(
        what="per-call wall clock through the Python mirror (ctypes) on one MI355X, host clock around calls that end in a stream "
             "wait; warm-up %d calls; compared variants alternate in one loop" % a.warmup,
        source="scripts/measure_frame_rgbd.py", device=torch.cuda.get_device_name(0),
        dev_flavour=dict(workload="2000 key points + 100 lines, 640 x 480, depth resident in HBM (tests/frame_rgbd_scenario.timing_inputs)",
                         **stats(t_dev)),
        host_flavours=dict(workload="the same through the two host flavours (two uploads of the 1.2 MB image)", **stats(t_host)),
        one_call=dict(workload="aloe_640x480.pgm, ORB 1000 features, EDLines 100 lines, TUM1 calibration, synthetic depth", **counts,
                      one_call=stats(t_one), sum_of_pieces=stats(total), pieces={k: stats(v) for k, v in t_pieces.items()}))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(doc, fh, indent=1)
    print(json.dumps(doc["gpu"], indent=1))


if __name__ == "__main__":
    main()
