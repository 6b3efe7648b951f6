#!/usr/bin/env python3
"""Per-call times of the stereo frame entries on the GPU -> profiles/frame_stereo_timing.json (beside the "cpu_reference" figure
scripts/make_frame_stereo_golden.py measured on one core):
  line_call     plvs_hip_frame_compute_stereo_line_matches, 100 + 100 lines (tests/frame_stereo_scenario.random_inputs(100, 100, 7))
  parent_knn    what the parent commit offers for the same work: plvs_hip_lines_search_stereo_by_knn (device k-NN, copy back, host
                pass) — WITHOUT the triangulation, which its caller runs on the host afterwards: a lower bound of that path
  one_call      plvs_hip_frame_stereo_dev against the sum of its pieces called one by one, the 1241 x 376 golden pair
Host clock around calls that end in a stream wait (the outputs are host arrays); warm-up first; the variants of a comparison
alternate inside one loop.  Usage: measure_frame_stereo.py [--calls 200] [--out profiles/frame_stereo_timing.json]"""
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
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "frame_stereo_timing.json"))
    a = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "a measurement needs the GPU"
    from plvs_amd import frame
    from plvs_amd.linematcher import LineMatcher
    from plvs_amd.lines import LineExtractor
    from plvs_amd.orb import ORBextractor
    from plvs_amd.stereo import StereoMatcher
    from tests import frame_stereo_scenario as S
    from tests.oracle_lib import golden
    from tests.test_frame_stereo import KITTI_BF, KITTI_K, _line_level_sigma2

    def clock(fn):
        t0 = time.perf_counter()
        fn()
        return (time.perf_counter() - t0) * 1e6

    kl, desc, klr, desc_r = S.random_inputs(100, 100, seed=7)
    al, ol, ar, orr = kl["angle"].copy(), kl["octave"].copy(), klr["angle"].copy(), klr["octave"].copy()
    matcher = LineMatcher(0.7, True)
    line_call = lambda: frame.compute_stereo_line_matches(kl, desc, klr, desc_r, S.LEVEL_SIGMA2, S.K4, S.MBF)          # noqa: E731
    parent = lambda: matcher.SearchStereoMatchesByKnn(desc, al, ol, desc_r, ar, orr, 50)                                # noqa: E731
    with_depth = line_call()[4]
    t_line, t_parent = [], []
    for k in range(a.warmup + a.calls):
        tl, tp = clock(line_call), clock(parent)
        if k >= a.warmup:
            t_line.append(tl)
            t_parent.append(tp)

    gl, gr = golden("urban1_1241x376.pgm"), golden("urban1_right_1241x376.pgm")
    h, w = gl.shape
    left, right = torch.from_numpy(gl).cuda(), torch.from_numpy(gr).cuda()
    b = frame.ComputeImageBounds(w, h, KITTI_K, None)
    gw, gh = np.float32(64) / (np.float32(b[1]) - np.float32(b[0])), np.float32(48) / (np.float32(b[3]) - np.float32(b[2]))
    orb_l, orb_r = ORBextractor(2000, 1.2, 8, 20, 7), ORBextractor(2000, 1.2, 8, 20, 7)
    lines_l, lines_r = LineExtractor(100), LineExtractor(100)
    sigma2 = _line_level_sigma2(lines_l.opts.numOctaves, lines_l.opts.scale)
    stereo = StereoMatcher(orb_l, orb_r)
    mbf = np.float32(KITTI_BF)
    mb = mbf / np.float32(KITTI_K[0])
    one = lambda: frame.frame_stereo(orb_l, orb_r, lines_l, lines_r, stereo, left, right, KITTI_K, None, KITTI_BF, b[:4], gw, gh,    # noqa: E731
                                     line_level_sigma2=sigma2)
    piece_names = ("extract_frame_left", "extract_frame_right", "UndistortKeyPoints", "ComputeStereoMatches", "ComputeStereoLineMatches",
                   "AssignFeaturesToGrid")
    t_one, t_pieces = [], {k: [] for k in piece_names}
    counts = None
    for k in range(a.warmup + a.calls):
        to = clock(one)
        t = [time.perf_counter()]
        mono, kps, d, kll, kld = frame.extract_frame(orb_l, lines_l, left)
        t.append(time.perf_counter())
        _, kr, dr, klr_, kldr = frame.extract_frame(orb_r, lines_r, right)
        t.append(time.perf_counter())
        un = frame.UndistortKeyPoints(kps, KITTI_K, None)
        t.append(time.perf_counter())
        stereo.ComputeStereoMatches(kps, d, kr, dr, mb, mbf)
        t.append(time.perf_counter())
        ns = frame.compute_stereo_line_matches(kll, kld, klr_, kldr, sigma2, KITTI_K, mbf)[4]
        t.append(time.perf_counter())
        frame.AssignFeaturesToGrid(un, b[0], b[2], gw, gh)
        t.append(time.perf_counter())
        counts = dict(key_points=len(kps), key_points_right=len(kr), lines=len(kll), lines_right=len(klr_), lines_with_depth=int(ns))
        if k >= a.warmup:
            t_one.append(to)
            for i, name in enumerate(piece_names):
                t_pieces[name].append((t[i + 1] - t[i]) * 1e6)
    total = np.sum([t_pieces[k] for k in piece_names], 0)
    doc = {}
    src = os.path.join(ROOT, "profiles", "frame_stereo_timing.json")
    if os.path.exists(src):
        with open(src) as fh:
            doc = json.load(fh)
    doc["gpu"] = dict(
        what="per-call wall clock through the Python mirror (ctypes) on one MI355X, host clock around calls that end in a stream "
             "wait; warm-up %d calls; compared variants alternate in one loop" % a.warmup,
        source="scripts/measure_frame_stereo.py", device=torch.cuda.get_device_name(0),
        line_call=dict(workload="100 + 100 lines (tests/frame_stereo_scenario.random_inputs(100, 100, 7)), %d left with depth" % with_depth,
                       **stats(t_line)),
        parent_knn=dict(workload="the same descriptors through plvs_hip_lines_search_stereo_by_knn: k-NN on the device, copy back, host "
                                 "pass; the triangulation its caller still has to run on the host is NOT included", **stats(t_parent)),
        one_call=dict(workload="urban1 pair 1241 x 376, ORB 2000 features, EDLines 100 lines a side, KITTI00-02 calibration; the pieces "
                               "extract the two sides one after the other, the one call side by side", **counts,
                      one_call=stats(t_one), sum_of_pieces=stats(total), pieces={k: stats(v) for k, v in t_pieces.items()}))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(doc, fh, indent=1)
    print(json.dumps(doc["gpu"], indent=1))


if __name__ == "__main__":
    main()
