"""The frame glue and the RGB-D part of include/plvs_hip.hpp: tests/host/frame_rgbd_smoke.cpp compiles against nothing but the C
ABI, and on the GPU its outputs equal the Python mirror's byte for byte (the Python path is what tests/test_frame_rgbd.py pins
to the reference)."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host", "frame_rgbd_smoke.cpp")


def build(out):
    lib_dir = os.path.join(ROOT, "plvs_amd", "lib")
    subprocess.run(["g++", "-std=c++14", "-O1", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), SRC,
                    "-L", lib_dir, "-l:libplvs_hip.so", "-Wl,-rpath," + lib_dir, "-Wl,-rpath,/opt/rocm/lib", "-o", out],
                   check=True)


def test_frame_rgbd_cpp_mirror_compiles_against_the_c_abi_only(tmp_path):
    build(str(tmp_path / "frame_rgbd_smoke"))


@pytest.mark.gpu
def test_frame_rgbd_cpp_mirror_matches_python_mirror(tmp_path):
    import torch
    from plvs_amd import frame
    from plvs_amd.lines import LineExtractor
    from plvs_amd.orb import ORBextractor
    from tests.oracle_lib import golden
    from tests.test_frame_rgbd import LINE_KEYS, MBF, TUM1_D, TUM1_K, _synthetic_depth
    exe = str(tmp_path / "frame_rgbd_smoke")
    build(exe)
    out = tmp_path / "out"
    out.mkdir()
    grey = golden("aloe_640x480.pgm")
    h, w = grey.shape
    pitch = 704
    depth = _synthetic_depth(h, w, pitch)
    depth.tofile(str(tmp_path / "depth.bin"))
    r = subprocess.run([exe, os.path.join(ROOT, "tests", "golden", "aloe_640x480.pgm"), str(tmp_path / "depth.bin"), str(pitch), str(out)],
                       check=True, capture_output=True, text=True)
    said = {l.split()[0]: l.split()[1:] for l in r.stdout.splitlines() if l}
    raw = lambda name: np.fromfile(str(out / (name + ".bin")), dtype=np.uint8).tobytes()      # noqa: E731

    # the steps one by one, host flavours, as the program does them
    orb, lines = ORBextractor(1000, 1.2, 8, 20, 7), LineExtractor(100)
    mono, keys, desc = orb(grey)
    kl, kld = lines(grey)
    b = frame.ComputeImageBounds(w, h, TUM1_K, TUM1_D)
    assert raw("bounds") == np.array(b, np.float32).tobytes()
    gw, gh = np.float32(64) / (np.float32(b[1]) - np.float32(b[0])), np.float32(48) / (np.float32(b[3]) - np.float32(b[2]))
    bounds4 = (b[0], float(np.float32(b[1]) - np.float32(60)), b[2], b[3])
    un = frame.UndistortKeyPoints(keys, TUM1_K, TUM1_D)
    image_view = depth[:, :w]
    ur, z = frame.ComputeStereoFromRGBD(keys, un, image_view, MBF)
    klu, kept = frame.UndistortKeyLines(kl, TUM1_K, TUM1_D, bounds4)
    ls = frame.ComputeStereoLinesFromRGBD(kl[kept], klu, image_view, TUM1_K, MBF)
    start, items = frame.AssignFeaturesToGrid(un, bounds4[0], bounds4[2], gw, gh)
    median = frame.ComputeSceneMedianDepth(z)
    steps = dict(keys=keys, keys_un=un, desc=desc, u_right=ur, depth=z, keylines=kl[kept], keylines_un=klu, line_desc=kld[kept],
                 cell_start=start, cell_items=items, **dict(zip(LINE_KEYS, ls)))
    assert [int(x) for x in said["steps"][:5]] == [mono, len(keys), len(kl), len(kept), len(items)]
    assert np.float32(float(said["steps"][5])) == median and 20 < len(kept) < len(kl) and len(keys) > 500
    for k, v in steps.items():
        assert raw("s_" + k) == np.ascontiguousarray(v).tobytes(), k

    # the constructor in one call
    got = frame.rgbd_frame(orb, lines, torch.from_numpy(grey).cuda(), torch.from_numpy(depth).cuda()[:, :w], TUM1_K, TUM1_D, MBF, bounds4,
                           gw, gh, use_median_depth=True)
    assert [int(x) for x in said["one_call"][:4]] == [got["mono_index"], len(got["keys"]), len(got["keylines"]), len(got["cell_items"])]
    assert np.float32(float(said["one_call"][4])) == got["median_depth"] == median
    names = dict(keys="keys", keys_un="keys_un", desc="descriptors", u_right="u_right", depth="depth", keylines="keylines",
                 keylines_un="keylines_un", line_desc="line_descriptors", cell_start="cell_start", cell_items="cell_items",
                 **{k: k for k in LINE_KEYS})
    for k, v in names.items():
        assert raw("f_" + k) == np.ascontiguousarray(got[v]).tobytes(), k
