"""The stereo part of include/plvs_hip.hpp: tests/host/frame_stereo_smoke.cpp compiles against nothing but the C ABI, and on the
GPU its outputs equal the Python mirror's byte for byte (the Python path is what tests/test_frame_stereo.py pins to the
reference).  The same program is built once more with the host side of plvs_amd/csrc/frame_stereo.hip under AddressSanitizer and
UBSan linked into it, and run as far as the argument checks that return before any HIP call: a stand-alone program, no GPU."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host", "frame_stereo_smoke.cpp")
LIB_DIR = os.path.join(ROOT, "plvs_amd", "lib")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def build(out):
    subprocess.run(["g++", "-std=c++14", "-O1", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), SRC,
                    "-L", LIB_DIR, "-l:libplvs_hip.so", "-Wl,-rpath," + LIB_DIR, "-Wl,-rpath,/opt/rocm/lib", "-o", out],
                   check=True)


def test_frame_stereo_cpp_mirror_compiles_and_refuses_bad_arguments(tmp_path):
    exe = str(tmp_path / "frame_stereo_smoke")
    build(exe)
    r = subprocess.run([exe, "--args-only"], capture_output=True, text=True)
    assert r.returncode == 0 and "args_only ok" in r.stdout, r.stdout + r.stderr


def test_argument_checks_under_host_sanitizers(tmp_path):
    """frame_stereo.hip's host code (argument checks, packing) with -fsanitize=address,undefined, linked into the stand-alone
    program in front of the library's copy; only paths that return before any HIP call run."""
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-g"]
    obj, exe = str(tmp_path / "frame_stereo_host.o"), str(tmp_path / "frame_stereo_smoke_san")
    csrc = os.path.join(ROOT, "plvs_amd", "csrc")
    subprocess.run([HIPCC, "--offload-arch=gfx950", "-O1", "-std=c++17", "-fPIC", "-ffp-contract=off", "-fno-fast-math",
                    "-I" + os.path.join(ROOT, "include"), *[x for f in san for x in ("-Xarch_host", f)], "-c", os.path.join(csrc, "frame_stereo.hip"), "-o", obj], check=True)
    subprocess.run([HIPCC, "-x", "c++", "-std=c++17", "-O1", *san, "-I" + os.path.join(ROOT, "include"), "-c", SRC, "-o", exe + ".o"],
                   check=True)
    subprocess.run([HIPCC, "--offload-arch=gfx950", *san, exe + ".o", obj, "-L" + LIB_DIR, "-l:libplvs_hip.so", "-Wl,-rpath," + LIB_DIR,
                    "-Wl,-rpath,/opt/rocm/lib", "-o", exe], check=True)
    r = subprocess.run([exe, "--args-only"], capture_output=True, text=True,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1"))
    assert r.returncode == 0 and "args_only ok" in r.stdout, r.stdout + r.stderr
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr


@pytest.mark.gpu
def test_frame_stereo_cpp_mirror_matches_python_mirror(tmp_path):
    import torch
    from plvs_amd import frame
    from plvs_amd.lines import LineExtractor
    from plvs_amd.orb import ORBextractor
    from plvs_amd.stereo import StereoMatcher
    from tests.oracle_lib import golden
    from tests.test_frame_stereo import KITTI_BF, KITTI_K, LINE_KEYS, _line_level_sigma2
    exe = str(tmp_path / "frame_stereo_smoke")
    build(exe)
    out = tmp_path / "out"
    out.mkdir()
    gold = os.path.join(ROOT, "tests", "golden")
    r = subprocess.run([exe, os.path.join(gold, "urban1_1241x376.pgm"), os.path.join(gold, "urban1_right_1241x376.pgm"), str(out)],
                       check=True, capture_output=True, text=True)
    said = {l.split()[0]: [int(x) for x in l.split()[1:]] for l in r.stdout.splitlines() if l}
    raw = lambda name: np.fromfile(str(out / (name + ".bin")), dtype=np.uint8).tobytes()      # noqa: E731
    gl, gr = golden("urban1_1241x376.pgm"), golden("urban1_right_1241x376.pgm")
    h, w = gl.shape
    orb_l, orb_r = ORBextractor(2000, 1.2, 8, 20, 7), ORBextractor(2000, 1.2, 8, 20, 7)
    lines_l, lines_r = LineExtractor(100), LineExtractor(100)
    sigma2 = _line_level_sigma2(3, 1.2)

    # the line call on separately extracted lines
    kl, kld = lines_l(gl)
    klr, kldr = lines_r(gr)
    *ls, ns = frame.compute_stereo_line_matches(kl, kld, klr, kldr, sigma2, KITTI_K, KITTI_BF)
    assert said["line_call"] == [len(kl), len(klr), ns] and ns >= 3
    steps = dict(keylines=kl, keylines_right=klr, line_desc=kld, line_desc_right=kldr, **dict(zip(LINE_KEYS, ls)))
    for k, v in steps.items():
        assert raw("s_" + k) == np.ascontiguousarray(v).tobytes(), k

    # the constructor in one call
    b = frame.ComputeImageBounds(w, h, KITTI_K, None)
    gw, gh = np.float32(64) / (np.float32(b[1]) - np.float32(b[0])), np.float32(48) / (np.float32(b[3]) - np.float32(b[2]))
    got = frame.frame_stereo(orb_l, orb_r, lines_l, lines_r, StereoMatcher(orb_l, orb_r), torch.from_numpy(gl).cuda(),
                             torch.from_numpy(gr).cuda(), KITTI_K, None, KITTI_BF, b[:4], gw, gh, line_level_sigma2=sigma2)
    assert said["one_call"] == [got["mono_index"], len(got["keys"]), len(got["keys_right"]), len(got["keylines"]), len(got["keylines_right"]),
                                len(got["cell_items"]), got["n_stereo_points"], got["n_stereo_lines"]]
    names = dict(keys="keys", keys_un="keys_un", desc="descriptors", u_right="u_right", depth="depth", keys_right="keys_right",
                 desc_right="descriptors_right", keylines="keylines", keylines_un="keylines_un", line_desc="line_descriptors",
                 keylines_right="keylines_right", keylines_right_un="keylines_right_un", line_desc_right="line_descriptors_right",
                 cell_start="cell_start", cell_items="cell_items", **{k: k for k in LINE_KEYS})
    for k, v in names.items():
        assert raw("f_" + k) == np.ascontiguousarray(got[v]).tobytes(), k
