"""libelas, the dense stereo matcher behind PointCloudKeyFrame::ProcessStereoLibelas (src/PointCloudKeyFrame.cc:335), is
the one component of the path's neighbourhood for which the reference tree STORES outputs:
Thirdparty/libelas-gpu/GPU_test/2016_12_06_cpu/*_disp.pgm for Thirdparty/libelas-gpu/input/*.pgm.  The CPU sources compile
unmodified (oracle/ref/Makefile -> oracle/_ref/libelas_ref.so); this test runs them over the reference's own inputs and
compares with the stored files as main_cpu.cpp wrote them (disparities scaled to 255 / max).  The stored files come from
another build of the library: validity masks are reproduced exactly, disparities to within one grey level for >= 98.5 %
of the pixels.  The tree's inputs and stored outputs of the two pairs are fixtures under tests/golden/libelas/ (its PGM
files, xz-compressed); the test is skipped where the library is absent.  The stages of libelas that run on the device
are checked in tests/test_elas.py; nothing on the GPU is checked here.  (The library is built with
oracle/ref/elas_zero_malloc.h in front of the sources: memory they read without having written it is zero, as in a fresh
process.)"""
import ctypes
import os

import numpy as np
import pytest

from tests.pgm import read_pgm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.path.join(ROOT, "oracle", "_ref", "libelas_ref.so")
TREE = os.path.join(ROOT, "tests", "golden", "libelas")      # input/*.pgm and GPU_test/2016_12_06_cpu/*_disp.pgm of the tree

pytestmark = pytest.mark.skipif(not os.path.exists(REF), reason="needs oracle/_ref/libelas_ref.so")


@pytest.mark.parametrize("name", ["cones", "raindeer"])
def test_compiled_libelas_against_the_outputs_the_reference_stores(name):
    lib = ctypes.CDLL(REF)
    lib.ref_elas_process.argtypes = [ctypes.c_void_p] * 2 + [ctypes.c_int] * 5 + [ctypes.c_void_p] * 2
    left, right = read_pgm(f"{TREE}/{name}_left.pgm.xz"), read_pgm(f"{TREE}/{name}_right.pgm.xz")
    h, w = left.shape
    d1, d2 = np.zeros((h, w), np.float32), np.zeros((h, w), np.float32)
    lib.ref_elas_process(left.ctypes.data, right.ctypes.data, w, h, w, 0, 0, d1.ctypes.data, d2.ctypes.data)
    dmax = float(max(d1.max(), d2.max()))
    for d, side in ((d1, "left"), (d2, "right")):
        out = np.maximum(255.0 * d.astype(np.float64) / dmax, 0.0).astype(np.uint8)      # main_cpu.cpp:76-79
        stored = read_pgm(f"{TREE}/{name}_{side}_disp.pgm.xz")
        assert np.array_equal(out > 0, stored > 0), f"{name} {side}: validity masks differ"
        close = np.abs(out.astype(int) - stored.astype(int)) <= 1
        assert close.mean() >= 0.985, f"{name} {side}: {1 - close.mean():.3%} of the pixels off by more than one level"
