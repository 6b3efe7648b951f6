#!/usr/bin/env python3
"""Golden outputs of the REFERENCE'S OWN Frame::ComputeStereoFromRGBD / ComputeStereoLinesFromRGBD /
ComputeSceneMedianDepth on tests/frame_rgbd_scenario.py: scripts/ref_wrap/frame_rgbd_ref_wrap.cpp — calls only — is compiled
into a temporary directory against oracle/_ref/libmatchers_ref.so (src/Frame.cc unmodified) with the include flags of
oracle/ref/Makefile's matchers target, and this script writes
  tests/golden/frame_rgbd_reference.npz          every output float of the reference's run + the inputs digest
  tests/golden/frame_rgbd_reference_facts.json   per-branch counts: the restatement's counters on the same run, taken only
                                                 after the restatement has reproduced the reference's floats bit for bit
It asserts ON THE REFERENCE'S RUN that the scenario takes every branch the tests rely on, and times the reference's two
functions on one core (profiles/frame_rgbd_timing.json, key "cpu_reference").  Dev-time tool: needs the reference tree and
the compiled reference library."""
import ctypes
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import frame_rgbd_restatement as R      # noqa: E402
from tests import frame_rgbd_scenario as S         # noqa: E402

MIN_PER_BRANCH = ("misaligned", "repaired_emax", "repaired_smax", "rejected", "short", "view_angle", "no_middle", "no_end_point")


def reference_root():
    """The reference tree: $PLVS_REFERENCE, or where oracle/ref/Makefile looks for it (its REF default)."""
    if os.environ.get("PLVS_REFERENCE"):
        return os.environ["PLVS_REFERENCE"]
    with open(os.path.join(ROOT, "oracle", "ref", "Makefile")) as f:
        for line in f:
            if line.startswith("REF") and "?=" in line:
                return line.split("?=", 1)[1].strip()
    raise SystemExit("set PLVS_REFERENCE to the reference tree")


def build_wrapper(tmp):
    ref, oref, rdir = reference_root(), os.path.join(ROOT, "oracle", "ref"), os.path.join(ROOT, "oracle", "_ref")
    ld = os.path.join(ref, "Thirdparty", "line_descriptor")
    inc = [os.path.join(oref, "slam_shim"), os.path.join(oref, "cv_full"), os.path.join(oref, "eigen_full"), os.path.join(ref, "include"),
           ref, os.path.join(ref, "include", "CameraModels"), os.path.join(ld, "include"), os.path.join(ld, "include", "line_descriptor"),
           os.path.join(ld, "src"), os.path.join(ref, "Thirdparty", "Sophus"), os.path.join(ROOT, "include"), oref]
    out = os.path.join(tmp, "libframe_rgbd_ref.so")
    subprocess.run(["g++", "-O2", "-std=c++14", "-fPIC", "-ffp-contract=off", "-fno-fast-math", "-w", *["-I" + i for i in inc],
                    "-include", os.path.join(oref, "slam_shim", "slam_shim.h"), "-shared",
                    os.path.join(ROOT, "scripts", "ref_wrap", "frame_rgbd_ref_wrap.cpp"), "-o", out, "-L" + rdir,
                    "-l:libmatchers_ref.so", "-Wl,-rpath," + rdir], check=True)
    return ctypes.CDLL(out)


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def ref_points(lib, inp, use_median):
    n = len(inp["kps"])
    ur, z, med = np.empty(n, np.float32), np.empty(n, np.float32), np.empty(2, np.float32)
    depth = np.ascontiguousarray(inp["depth"])
    lib.ref_frame_stereo_from_rgbd(_p(inp["kps"]), _p(inp["kps_un"]), n, _p(depth), inp["width"], inp["height"], inp["pitch"],
                                   ctypes.c_float(float(inp["mbf"])), int(use_median), _p(ur), _p(z), _p(med))
    return ur, z, med


def ref_lines(lib, inp):
    n = len(inp["keylines"])
    out = [np.empty(n, np.float32) for _ in range(4)]
    depth, K4 = np.ascontiguousarray(inp["depth"]), np.ascontiguousarray(inp["K4"], np.float32)
    lib.ref_frame_stereo_lines_from_rgbd(_p(inp["keylines"]), _p(inp["keylines_un"]), n, _p(depth), inp["width"], inp["height"],
                                         inp["pitch"], _p(K4), ctypes.c_float(float(inp["mbf"])),
                                         ctypes.c_float(float(inp["min_line_length_3d"])), *[_p(o) for o in out])
    return out


def same_bits(a, b):
    return np.array_equal(np.asarray(a, np.float32).view(np.uint32), np.asarray(b, np.float32).view(np.uint32))


def time_reference(lib):
    inp = S.timing_inputs()
    pts, lns = [], []
    for k in range(60):
        t0 = time.perf_counter()
        ref_points(lib, inp, 0)
        t1 = time.perf_counter()
        ref_lines(lib, inp)
        t2 = time.perf_counter()
        if k >= 10:
            pts.append((t1 - t0) * 1e6)
            lns.append((t2 - t1) * 1e6)
    return dict(what="Frame::ComputeStereoFromRGBD + Frame::ComputeStereoLinesFromRGBD of the reference (src/Frame.cc as "
                     "oracle/_ref/libmatchers_ref.so builds it: -O2, no contraction), one core, 2000 key points and 100 lines on "
                     "640 x 480 (tests/frame_rgbd_scenario.timing_inputs), wall clock per call incl. filling the Frame; median of 50",
                source="scripts/make_frame_rgbd_golden.py", us_points_median=round(float(np.median(pts)), 1),
                us_lines_median=round(float(np.median(lns)), 1), us_both_median=round(float(np.median(np.add(pts, lns))), 1))


def main():
    inp = S.inputs()
    with tempfile.TemporaryDirectory() as tmp:
        lib = build_wrapper(tmp)
        ur, z, med = ref_points(lib, inp, 1)
        _, _, med_off = ref_points(lib, inp, 0)
        line_out = ref_lines(lib, inp)
        timing = time_reference(lib)
    # the restatement beside the reference: bit for bit, then its counters are the reference's branch counts
    xy = np.stack([inp["kps"]["x"], inp["kps"]["y"]], -1)
    r_ur, r_z = R.stereo_from_rgbd(xy, inp["kps_un"]["x"], S.image_of(inp), inp["mbf"])
    assert same_bits(r_ur, ur) and same_bits(r_z, z), "points: the restatement differs from the reference"
    assert same_bits(R.scene_median_depth(z), med[0]) and same_bits(med[0], med[1]) and med_off[0] == np.float32(1.5)
    counters = {}
    r_lines = R.stereo_lines_from_rgbd(S.lines8(inp), S.image_of(inp), inp["K4"], inp["mbf"], inp["min_line_length_3d"], counters)
    bad = sum(int((np.asarray(a).view(np.uint32) != np.asarray(b).view(np.uint32)).sum()) for a, b in zip(r_lines, line_out))
    assert bad == 0, f"lines: the restatement differs from the reference in {bad} floats"
    stereo = int((line_out[1] > 0).sum())
    facts = dict(lines=len(inp["keylines"]), points=len(inp["kps"]), **{k: int(v) for k, v in counters.items()},
                 points_without_depth=int((z < 0).sum()), points_inf=int(np.isinf(z).sum()))
    assert stereo == counters["stereo"] and all((line_out[1] > 0) == (line_out[3] > 0))
    for k in MIN_PER_BRANCH:
        assert facts[k] >= 5, f"only {facts[k]} lines take the branch {k}"
    assert facts["stereo"] >= 150 and facts["points_without_depth"] >= 20 and facts["points_inf"] >= 3, facts
    gdir = os.path.join(ROOT, "tests", "golden")
    np.savez_compressed(os.path.join(gdir, "frame_rgbd_reference.npz"), u_right=ur, depth=z, median=med[:1],
                        u_right_start=line_out[0], depth_start=line_out[1], u_right_end=line_out[2], depth_end=line_out[3],
                        inputs_digest=np.array(S.inputs_digest(inp)))
    with open(os.path.join(gdir, "frame_rgbd_reference_facts.json"), "w") as fh:
        json.dump(dict(what="branch counts of the reference's Frame::ComputeStereoLinesFromRGBD / ComputeStereoFromRGBD on "
                            "tests/frame_rgbd_scenario.py (see scripts/make_frame_rgbd_golden.py)",
                       inputs=S.inputs_digest(inp), facts=facts), fh, indent=1)
    tpath = os.path.join(ROOT, "profiles", "frame_rgbd_timing.json")
    doc = {}
    if os.path.exists(tpath):
        with open(tpath) as fh:
            doc = json.load(fh)
    doc["cpu_reference"] = timing
    with open(tpath, "w") as fh:
        json.dump(doc, fh, indent=1)
    print(facts, timing)


if __name__ == "__main__":
    main()
